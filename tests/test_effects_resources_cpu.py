"""The resource figures the post-effect kernels' design rests on (sailor_amd/csrc/post_effects.hip), read from the AMDGPU metadata of the built code object
like tests/test_tail_resources_cpu.py: the expected kernels and no others, no scratch, no spills and no LDS (one texel per lane, nothing shared),
256-thread blocks, and the eight waves per SIMD DESIGN.md states for each of them -- all are gathers bound by memory latency, so full occupancy is what
hides it.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "post_effects.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_post_effects"))


def test_the_expected_kernels_and_no_others(resources):
    names = list(resources)
    for kernel, count in (("k_blur_gauss", 1), ("k_blur_radial", 1), ("k_chromatic_aberration", 1), ("k_blit_linear", 2)):   # the blit: one and four channels
        assert sum(kernel in n for n in names) == count, (kernel, names)
    assert len(names) == 5, names


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    for name, k in resources.items():
        print(f"{name}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs")
        assert waves_per_simd(k["vgpr_count"]) == 8, (name, k["vgpr_count"])
    assert find(resources, "k_blur_gauss")["vgpr_count"] <= 64
