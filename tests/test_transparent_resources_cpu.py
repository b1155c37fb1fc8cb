"""The resource figures the Transparent queue's kernels rest on (sailor_amd/csrc/surface_transparent.hip), read from the AMDGPU metadata of the built code object
like tests/test_lod_resources_cpu.py: the expected kernels and no others, no scratch, no vector spills and no LDS, 256-thread blocks, the scalar spills
DESIGN.md records (4 in k_surface_peel, to vector lanes; none in k_surface_peel_gltf, whose two plane pointers are kept in vector registers) and the occupancy
it records.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

SGPR_SPILLS = {"k_surface_peel": 4}   # the rest: none
WAVES = {"k_surface_peel": 3, "k_surface_peel_gltf": 2, "k_surface_peel_commit": 8, "k_surface_blend": 8}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "surface_transparent.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_surface_transparent"))


def test_the_expected_kernels_and_no_others(resources):
    for kernel in WAVES:
        find(resources, kernel)
    assert len(resources) == len(WAVES), list(resources)


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["sgpr_spill_count"] == next((n for kernel, n in SGPR_SPILLS.items() if k is find(resources, kernel)), 0), (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    for kernel, want in WAVES.items():
        k = find(resources, kernel)
        print(f"{kernel}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['sgpr_spill_count']} SGPR spills")
        assert waves_per_simd(k["vgpr_count"]) == want, (kernel, k["vgpr_count"])
