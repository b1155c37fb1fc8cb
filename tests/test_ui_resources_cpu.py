"""The resource figures the RenderImGui pass's kernels rest on (sailor_amd/csrc/ui_draw.hip), read from the AMDGPU metadata of the built code object like
tests/test_lines_resources_cpu.py: the three expected kernels and no others, no scratch and no spills, 256-thread blocks, the LDS of the blend's ordered list
(and of the scan's four wave sums) and the occupancy DESIGN.md records.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

WAVES = {"k_ui_scan": 8, "k_ui_setup": 8, "k_ui_blend": 4}
# k_ui_blend: 256 list entries of 80 bytes (a 16-byte box and a 64-byte record), four wave counts and the table of the 256 quotients byte / 255;
# k_ui_scan: four 64-bit wave sums; k_ui_setup: none
LDS = {"k_ui_scan": 32, "k_ui_setup": 0, "k_ui_blend": 256 * 80 + 16 + 256 * 4}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "ui_draw.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_ui_draw"))


def test_the_expected_kernels_and_no_others(resources):
    for kernel in WAVES:
        find(resources, kernel)
    assert len(resources) == len(WAVES), list(resources)


def test_no_kernel_uses_scratch_or_spills_and_lds_is_what_the_design_states(resources):
    for kernel, lds in LDS.items():
        k = find(resources, kernel)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (kernel, k)
        assert k["group_segment_fixed_size"] == lds and k["max_flat_workgroup_size"] == 256, (kernel, k)


def test_occupancy_the_design_states(resources):
    for kernel, waves in WAVES.items():
        k = find(resources, kernel)
        print(f"{kernel}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['group_segment_fixed_size']} bytes of LDS")
        assert waves_per_simd(k["vgpr_count"]) == waves, (kernel, k["vgpr_count"])
    # the blend's LDS admits more blocks per CU (160 KiB / 21 520 bytes = 7) than its registers do (4 waves per SIMD = 4 blocks of 4 waves): registers bound it
    assert (160 * 1024) // LDS["k_ui_blend"] >= 4
