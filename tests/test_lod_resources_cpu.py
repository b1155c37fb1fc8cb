"""The resource figures the mip-mapped kernels rest on (sailor_amd/csrc/texture_mips.hip, surface_lod.hip), read from the AMDGPU metadata of the built code
objects like tests/test_gltf_resources_cpu.py: the expected kernels and no others, no scratch, no vector spills and no LDS, 256-thread blocks, the scalar spills
DESIGN.md records (15 in each of the four draws, to vector lanes), and the occupancy it records.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

WAVES = {
    "texture_mips": {"k_texture_mip_down": 8},
    "surface_lod": {"k_surface_visibility_lod": 2, "k_surface_visibility_lod_gltf": 2, "k_surface_visibility_indirect_lod": 2,
                    "k_surface_visibility_indirect_lod_gltf": 2, "k_surface_resolve_lod": 3},
}
SGPR_SPILLS = {"k_surface_visibility": 15}   # kernel name contains -> the count DESIGN.md records (the four draws); absent = 0


@pytest.fixture(scope="module", params=sorted(WAVES))
def resources(request, tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / f"{request.param}.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return WAVES[request.param], kernel_resources(obj, tmp_path_factory.mktemp(f"co_{request.param}"))


def test_the_expected_kernels_and_no_others(resources):
    waves, res = resources
    for kernel in waves:
        find(res, kernel)
    assert len(res) == len(waves), list(res)


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    _, res = resources
    for name, k in res.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["sgpr_spill_count"] == next((n for kernel, n in SGPR_SPILLS.items() if kernel in name), 0), (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    waves, res = resources
    for kernel, want in waves.items():
        k = find(res, kernel)
        print(f"{kernel}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['sgpr_spill_count']} SGPR spills")
        assert waves_per_simd(k["vgpr_count"]) == want, (kernel, k["vgpr_count"])
