"""The resource figures the EyeAdaptation kernels' design rests on (sailor_amd/csrc/eye_adaptation.hip), read from the AMDGPU metadata of the built
code object like tests/test_kernel_resources_cpu.py: no scratch and no spills anywhere; the histogram's 64 KiB of LDS and 16-wave blocks let a CU hold
the two blocks (32 waves, all its SIMDs can run) the launch asks for; the streaming tone-map kernels stay at eight waves per SIMD.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "eye_adaptation.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_eye"))


def test_no_kernel_uses_scratch_or_spills(resources):
    names = list(resources)
    assert sum("k_tonemap" in n for n in names) == 6, names   # the six distinct operator bodies
    assert len(names) == 9, names                               # + histogram, average, reset
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)


def test_histogram_lds_allows_the_stated_occupancy(resources):
    k = find(resources, "k_luminance_histogram")
    # 16 waves x 256 bins x 4 replicas x 4 bytes
    assert k["group_segment_fixed_size"] == 16 * 256 * 4 * 4 and k["max_flat_workgroup_size"] == 1024
    blocks_by_lds = (160 * 1024) // k["group_segment_fixed_size"]
    blocks_by_waves = 4 * waves_per_simd(k["vgpr_count"]) // 16   # a 16-wave block puts four waves on each of the four SIMDs
    assert blocks_by_lds == 2 and blocks_by_waves == 2, (blocks_by_lds, blocks_by_waves, k)   # EA_BLOCKS_PER_CU = 2: 32 waves per CU


def test_average_is_one_small_block(resources):
    k = find(resources, "k_average_luminance")
    assert k["group_segment_fixed_size"] == 256 * 4 and k["max_flat_workgroup_size"] == 256


def test_tonemap_kernels_keep_eight_waves_per_simd(resources):
    for name, k in resources.items():
        if "k_tonemap" in name:
            assert waves_per_simd(k["vgpr_count"]) == 8 and k["group_segment_fixed_size"] == 0, (name, k)
