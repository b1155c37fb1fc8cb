"""The resource figures DESIGN.md states for the multisampled pass's kernels (sailor_amd/csrc/surface_msaa.hip), read from the AMDGPU metadata of the built code
object like tests/test_transparent_buckets_resources_cpu.py: the expected kernels and no others, no scratch, no vector spills and no LDS, 256-thread blocks, the
scalar spills (to vector lanes) of the two draw kernels, and the occupancy the build gives -- there was no preset target: 2 waves per SIMD for the draws (193 and
195 registers, 25 more than the masked draw they extend), 8 for the four lane-per-pixel kernels.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, kernel_resources, waves_per_simd

SGPR_SPILLS = {"k_surface_msaa": 23, "k_surface_msaa_gltf": 23, "k_surface_msaa_begin": 0, "k_surface_msaa_layer": 0, "k_surface_msaa_accumulate": 0,
               "k_surface_msaa_store_depth": 0}
WAVES = {"k_surface_msaa": 2, "k_surface_msaa_gltf": 2, "k_surface_msaa_begin": 8, "k_surface_msaa_layer": 8, "k_surface_msaa_accumulate": 8,
         "k_surface_msaa_store_depth": 8}


def named(resources, kernel):
    """the kernel of exactly this name (k_surface_msaa is a prefix of the others)"""
    hits = [k for name, k in resources.items() if f"{len(kernel)}{kernel}" in name]
    assert len(hits) == 1, (kernel, list(resources))
    return hits[0]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "surface_msaa.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_surface_msaa"))


def test_the_expected_kernels_and_no_others(resources):
    for kernel in WAVES:
        named(resources, kernel)
    assert len(resources) == len(WAVES), list(resources)


def test_no_kernel_uses_scratch_vector_spills_or_lds(resources):
    for kernel, spills in SGPR_SPILLS.items():
        k = named(resources, kernel)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == spills, (kernel, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (kernel, k)


def test_occupancy_the_design_states(resources):
    for kernel, want in WAVES.items():
        k = named(resources, kernel)
        print(f"{kernel}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['sgpr_spill_count']} SGPR spills")
        assert waves_per_simd(k["vgpr_count"]) == want, (kernel, k["vgpr_count"])
    assert named(resources, "k_surface_msaa")["vgpr_count"] == 193 and named(resources, "k_surface_msaa_gltf")["vgpr_count"] == 195
