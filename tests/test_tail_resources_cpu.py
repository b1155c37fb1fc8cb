"""The resource figures the tail kernels' design rests on (sailor_amd/csrc/post_tail.hip), read from the AMDGPU metadata of the built code object like
tests/test_hbao_resources_cpu.py: no scratch, no spills and no LDS anywhere (one texel per lane, nothing shared), 256-thread blocks, and the eight waves
per SIMD DESIGN.md states for all five kernels -- both passes are bound by memory latency, so full occupancy is what hides it.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "post_tail.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_post_tail"))


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    names = list(resources)
    assert sum("k_debug_view" in n for n in names) == 4, names   # SCENE, AO, LIGHT_TILES, CASCADES
    assert sum("k_motion_blur" in n for n in names) == 1 and len(names) == 5, names
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    for name, k in resources.items():
        assert waves_per_simd(k["vgpr_count"]) == 8, (name, k["vgpr_count"])
    assert find(resources, "k_motion_blur")["vgpr_count"] <= 64
