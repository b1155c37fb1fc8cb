"""The resource figures the sky kernels' design rests on (sailor_amd/csrc/sky.hip), read from the AMDGPU metadata of the built code object like
tests/test_kernel_resources_cpu.py: no scratch, no spills and no LDS anywhere (the wave-per-texel march exchanges its partial sums through
cross-lane moves only); the march keeps six waves per SIMD -- its dependent exponential chains want other waves to issue between them --, the sun
and compose kernels eight.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "sky.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_sky"))


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    names = list(resources)
    assert sum("k_sky_march" in n for n in names) == 2, names   # FILL (Earth test) and ENV
    assert len(names) == 4, names                                 # + k_sky_sun, k_sky_compose
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    for name, k in resources.items():
        if "k_sky_march" in name:
            assert k["vgpr_count"] <= 80 and waves_per_simd(k["vgpr_count"]) >= 6, (name, k)
    assert waves_per_simd(find(resources, "k_sky_sun")["vgpr_count"]) == 8
    assert waves_per_simd(find(resources, "k_sky_compose")["vgpr_count"]) == 8
