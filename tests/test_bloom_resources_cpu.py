"""The resource figures the bloom kernels' design rests on (sailor_amd/csrc/bloom.hip), read from the AMDGPU metadata of the built code object like
tests/test_kernel_resources_cpu.py: one output texel per lane and nothing shared between lanes -- no LDS (the reference's 10 x 10 tile and its barrier
are gone), no scratch, no spills; nine float4 taps in flight want the latency hidden, so all three bodies stay at eight waves per SIMD.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "bloom.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_bloom"))


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    names = list(resources)
    assert sum("k_bloom_upscale" in n for n in names) == 2, names   # with and without the dirt term
    assert len(names) == 3, names                                     # + k_bloom_downscale
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    assert waves_per_simd(find(resources, "k_bloom_downscale")["vgpr_count"]) == 8
    for name, k in resources.items():
        assert waves_per_simd(k["vgpr_count"]) == 8, (name, k)
