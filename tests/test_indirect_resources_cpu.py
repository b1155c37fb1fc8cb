"""The resource figures the indirect draw kernels rest on (sailor_amd/csrc/surface_indirect.hip), read from the AMDGPU metadata of the built code object like
tests/test_masked_resources_cpu.py: the two expected kernels and no others, no scratch, no spills and no LDS, 256-thread blocks, and the occupancy DESIGN.md
records -- both are surface_masked_body.h's draw behind one uniform load and a clamp, and sit at the three waves per SIMD of the two direct instantiations
(166 and 168 registers; built without the SLP vectoriser like them, see the Makefile).  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

WAVES = {"k_surface_visibility_indirect": 3, "k_surface_visibility_indirect_gltf": 3}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "surface_indirect.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_surface_indirect"))


def test_the_expected_kernels_and_no_others(resources):
    for kernel in WAVES:
        find(resources, kernel)
    assert len(resources) == len(WAVES), list(resources)


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    for kernel, waves in WAVES.items():
        k = find(resources, kernel)
        print(f"{kernel}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs")
        assert waves_per_simd(k["vgpr_count"]) == waves, (kernel, k["vgpr_count"])
