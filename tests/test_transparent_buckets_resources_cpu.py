"""The resource figures DESIGN.md states for the bucket route's kernels (sailor_amd/csrc/surface_buckets.hip), read from the AMDGPU metadata of the built code
object like tests/test_transparent_resources_cpu.py: the expected kernels and no others, no scratch, no vector spills and no LDS, 256-thread blocks, 15 scalar
spills (to vector lanes) in each draw kernel, and the occupancy: the Standard draw keeps its siblings' 3 waves per SIMD with both shortcuts of the insertion
taken.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

SGPR_SPILLS = {"k_surface_bucket_layer": 0, "k_surface_bucket_gltf": 15, "k_surface_bucket": 15}
WAVES = {"k_surface_bucket_layer": 8, "k_surface_bucket_gltf": 2, "k_surface_bucket": 3}


def named(resources, kernel):
    """the kernel of exactly this name (k_surface_bucket is a prefix of the other two)"""
    hits = [k for name, k in resources.items() if f"{len(kernel)}{kernel}" in name]
    assert len(hits) == 1, (kernel, list(resources))
    return hits[0]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "surface_buckets.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_surface_buckets"))


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
