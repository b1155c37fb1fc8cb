"""The resource figures of the shadow pass's instance gather (sailor_amd/csrc/shadow_instances.hip), read from the AMDGPU metadata of the built code object
like tests/test_indirect_resources_cpu.py: the three expected kernels and no others, compiled for gfx950 with no scratch and no spills -- the jobs travel by value
in the kernel arguments and are indexed by the block's number, which must stay a scalar load and not become a private copy --, the block sizes and LDS the file
states (the gather: 2 KiB of source indices + 16 counters; its scan: 16 wave totals + a carry; the position extraction: none), and the register counts in the message.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

# kernel -> (threads per block, LDS bytes)
KERNELS = {"k_shadow_gather_scan": (1024, 16 * 4 + 4), "k_shadow_gather": (256, 1024 * 2 + 16 * 4), "k_shadow_positions": (256, 0)}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "shadow_instances.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_shadow_instances"))


def test_the_expected_kernels_and_no_others(resources):
    for kernel in KERNELS:
        find(resources, kernel)
    assert len(resources) == len(KERNELS), list(resources)


def test_no_kernel_uses_scratch_or_spills(resources):
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)


def test_block_sizes_lds_and_register_counts(resources):
    figures = []
    for kernel, (threads, lds) in KERNELS.items():
        k = find(resources, kernel)
        figures.append(f"{kernel}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['group_segment_fixed_size']} B LDS, "
                       f"{waves_per_simd(k['vgpr_count'])} waves per SIMD by registers")
    message = "; ".join(figures)
    print(message)
    for kernel, (threads, lds) in KERNELS.items():
        k = find(resources, kernel)
        assert k["max_flat_workgroup_size"] == threads and k["group_segment_fixed_size"] == lds, (kernel, k, message)
        # both are bandwidth kernels: nothing in them may cost occupancy (a 1 024-thread block needs 4 waves per SIMD to start at all)
        assert waves_per_simd(k["vgpr_count"]) == 8, message
