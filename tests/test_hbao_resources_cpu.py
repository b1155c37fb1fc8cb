"""The resource figures the HBAO kernels' design rests on (sailor_amd/csrc/hbao.hip), read from the AMDGPU metadata of the built code object like
tests/test_kernel_resources_cpu.py: no scratch, no spills and no LDS anywhere (one texel per lane, nothing shared); the HBAO pass stays at seven
waves per SIMD -- its 70 gathers per texel want the latency hidden --, the blit and the two blur bodies at eight.  No GPU needed."""
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "hbao.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_hbao"))


def test_no_kernel_uses_scratch_spills_or_lds(resources):
    names = list(resources)
    assert sum("k_hbao_blur" in n for n in names) == 2, names   # VERTICAL and HORIZONTAL
    assert len(names) == 4, names                                 # + k_blit_nearest, k_hbao
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_design_states(resources):
    hbao = [k for n, k in resources.items() if "k_hbao" in n and "blur" not in n]
    assert len(hbao) == 1 and waves_per_simd(hbao[0]["vgpr_count"]) == 7, hbao
    assert waves_per_simd(find(resources, "k_blit_nearest")["vgpr_count"]) == 8
    for name, k in resources.items():
        if "k_hbao_blur" in name:
            assert waves_per_simd(k["vgpr_count"]) == 8, (name, k)
