"""The resource figures the clouds kernels' design states (sailor_amd/csrc/sky_clouds.hip), read from the AMDGPU metadata of the built
code object like tests/test_sky_resources_cpu.py: no scratch and no spills anywhere; the march keeps its per-octave phase terms in 10 x 256 floats of LDS
(an array indexed by the loop counter would otherwise live in scratch) and stays within 128 registers, four waves per SIMD; the sun and blit kernels use no
LDS and run at eight.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "sky_clouds.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_sky_clouds"))


def test_three_kernels_without_scratch_or_spills(resources):
    assert len(resources) == 3, list(resources)
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["max_flat_workgroup_size"] == 256, (name, k)


def test_registers_and_lds_the_design_states(resources):
    march = find(resources, "k_sky_clouds")
    assert march["group_segment_fixed_size"] == 10 * 256 * 4, march          # s_phase[10][256]
    assert march["vgpr_count"] <= 128 and waves_per_simd(march["vgpr_count"]) >= 4, march
    for name in ("k_sky_sun_clouds", "k_sky_blit_clouds"):
        k = find(resources, name)
        assert k["group_segment_fixed_size"] == 0 and waves_per_simd(k["vgpr_count"]) == 8, (name, k)
