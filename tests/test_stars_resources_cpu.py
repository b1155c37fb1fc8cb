"""The resource figures the header of sailor_amd/csrc/sky_stars.hip states, read from the AMDGPU metadata of the built code object like
tests/test_clouds_resources_cpu.py: three kernels, no scratch and no spills anywhere, a flat workgroup size of 256, no LDS, and eight waves per SIMD for the
sun-shaft pass and for both star kernels.  No GPU needed."""
import re
import shutil

import pytest

from test_kernel_resources_cpu import CSRC, LLVM, find, kernel_resources, waves_per_simd

KERNELS = ("k_sky_sun_shafts", "k_sky_stars_project", "k_sky_stars_blend")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (LLVM / "clang-offload-bundler").exists() or not shutil.which("objcopy"):
        pytest.skip("no ROCm LLVM tools here")
    obj = CSRC / "sky_stars.o"
    assert obj.exists(), f"{obj} is missing: run __graft_entry__.build()"
    return kernel_resources(obj, tmp_path_factory.mktemp("co_sky_stars"))


def test_three_kernels_without_scratch_or_spills(resources):
    assert len(resources) == 3, list(resources)
    for name, k in resources.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["max_flat_workgroup_size"] == 256, (name, k)


def test_occupancy_the_header_states(resources):
    header = (CSRC / "sky_stars.hip").read_text().split("#include")[0]
    stated = {name: int(m.group(1)) for name in KERNELS for m in [re.search(name + r": (\d) waves per SIMD", header)] if m}
    assert stated == {name: 8 for name in KERNELS}, stated
    for name in KERNELS:
        k = find(resources, name)
        assert k["group_segment_fixed_size"] == 0 and waves_per_simd(k["vgpr_count"]) == stated[name], (name, k)
