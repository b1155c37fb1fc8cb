"""The Transparent render queue without a GPU: the C-ABI's symbols, constants and version and the refusals a NULL context reaches; every other refusal, and
that the older draw entries refuse the blend bits, in the stand-alone scripts/transparent_host_check.cpp, which a test here builds and runs (and on the device
in tests/test_transparent_gpu.py); the restatement (tests/transparent_ref.py) held to float64 on every case of tests/transparent_cases.py with what each case
reaches counted; the measured error of the fp32 restatement chain; and five mutants of the restatement, each caught by a named case."""
import re
from pathlib import Path

import numpy as np
import pytest

import transparent_cases as cases
import transparent_ref as tr
from sailor_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("sailor_hip_surface_peel_begin", "sailor_hip_surface_peel_draw", "sailor_hip_surface_peel_draw_gltf", "sailor_hip_surface_peel_commit",
           "sailor_hip_surface_blend")


def test_abi_symbols_constants_version_and_null_context_refusals():
    lib = _lib.load()
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    assert lib.sailor_hip_version() >= 12
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"SAILOR_HIP_API int {name}(" in header, name
    define = lambda name: int(re.search(rf"#define {name} (\d+)u", header).group(1))
    assert (define("SAILOR_SURFACE_BLEND_SHIFT"), define("SAILOR_SURFACE_BLEND_MASK")) == (_lib.SURFACE_BLEND_SHIFT, _lib.SURFACE_BLEND_MASK) == (3, 3)
    assert [define(f"SAILOR_SURFACE_BLEND_{m}") for m in ("NONE", "ADDITIVE", "ALPHA", "MULTIPLY")] == [0, 1, 2, 3]
    assert [_lib.SURFACE_BLEND_MODES[m] for m in ("none", "additive", "alpha", "multiply")] == [0, 1, 2, 3]
    old = _lib.SURFACE_CULL_BACK | _lib.SURFACE_ALPHA_CUTOUT | _lib.SURFACE_GLTF
    assert (_lib.SURFACE_BLEND_MASK << _lib.SURFACE_BLEND_SHIFT) & old == 0 and (_lib.SURFACE_BLEND_MASK << _lib.SURFACE_BLEND_SHIFT) == old + 1 + 16
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [8, 16, 16, 8, 10]
    band = _lib.Band()
    assert lib.sailor_hip_surface_peel_begin(None, 8, 8, band, None, 0, None, 1) == -1
    assert lib.sailor_hip_surface_peel_draw(None, None, None, None, None, 0, None, 0, 0, 8, 8, band, None, 0, None, None) == -1
    assert lib.sailor_hip_surface_peel_draw_gltf(None, None, None, None, None, 0, None, 0, 0, 8, 8, band, None, 0, None, None) == -1
    assert lib.sailor_hip_surface_peel_commit(None, 8, 8, band, None, 0, None, None) == -1
    assert lib.sailor_hip_surface_blend(None, None, None, None, None, 0, None, 8, 8, band) == -1


def test_the_older_draw_entries_exclude_the_blend_bits_from_what_they_accept():
    """their `allowed` masks are spelled out flag by flag (no ~0, no blend field): read from the sources; the refusals themselves run in
    scripts/transparent_host_check.cpp and in tests/test_transparent_gpu.py"""
    csrc = ROOT / "sailor_amd" / "csrc"
    seen = 0
    for unit in ("surface.hip", "surface_masked.hip", "surface_gltf.hip", "surface_indirect.hip", "surface_lod.hip"):
        for call in re.findall(r"surf_draw_(?:prologue|launch)\(ctx, \"(\w+)\", ([^,]+),", (csrc / unit).read_text()):  # (_launch: the prologue and the launch behind it)
            flags = [f.strip() for f in call[1].split("|")]
            assert set(flags) <= {"SAILOR_SURFACE_CULL_BACK", "SAILOR_SURFACE_ALPHA_CUTOUT", "SAILOR_SURFACE_GLTF"}, call
            seen += 1
    assert seen == 6


def test_every_host_side_refusal_in_the_stand_alone_program(tmp_path):
    """scripts/transparent_host_check.cpp -- every refusal of the five entries and the older draw entries' refusal of the blend bits, against a context that
    never reaches a device -- built as a program of its own with the host sanitizers and run (a few seconds)"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "sailor_amd" / "csrc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc here")
    exe = tmp_path / "transparent_host_check"
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", f"-I{csrc}", str(ROOT / "scripts" / "transparent_host_check.cpp"), "-o", str(exe), f"-L{csrc}", "-lsailor_hip",
                            f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "transparent_host_check: ok" in run.stdout, run.stdout + run.stderr


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def restated(scenes):
    """name -> (depth attachment, layers, stats, the fp32 chain, the float64 chain): computed once, shared, left unchanged"""
    out = {}
    for name, s in scenes.items():
        depth = cases.depth_attachment(s)
        L, st = tr.layers(s, depth, count=True)
        s32, s64 = cases.shaders(s, depth)
        out[name] = (depth, L, st, tr.composite(L, s32, cases.target_of(s), np.float32), tr.composite(L, s64, cases.target_of(s), np.float64))
    return out


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_restatement_against_float64_and_what_the_case_reaches(scenes, restated, name):
    s = scenes[name]
    depth, L, st, c32, c64 = restated[name]
    assert s["W"] * s["H"] <= 50 * 35 and sum(len(d["indices"]) for d in s["draws"]) <= 16
    print(f"[{name}] layers per pixel {np.bincount(st['per_pixel'].ravel()).tolist()}, rejected by depth {st['rejected']}, discarded {st['discarded']}")
    assert cases.CASES[name][1](L, st, s), f"{name} does not reach what it was built for"
    for k, l in enumerate(L):   # a layer's orders ascend from layer to layer at every pixel, and a pixel without a k-th fragment has no later one
        assert (l["covered"] == (l["last"] != 0)).all()
        if k:
            assert (l["last"][l["covered"]] > L[k - 1]["last"][l["covered"]]).all() and not (l["covered"] & ~L[k - 1]["covered"]).any()
    finite = np.isfinite(c64)
    assert (np.isnan(c32) == np.isnan(c64)).all() and (np.isinf(c32) == np.isinf(c64)).all(), "non-finite channels differ in class"
    tol = cases.chain_tolerance(L, cases.shaders(s, depth)[1], cases.target_of(s))
    with np.errstate(all="ignore"):
        err = np.abs(c32.astype(np.float64) - c64)
        touched = (st["per_pixel"] > 0)[..., None] & finite
        ratio = np.nanmax(err[touched] / tol[touched])   # (0 / 0 where a channel is copied exactly: the alpha of blend None)
    print(f"[{name}] worst |c32 - c64| {err[touched].max():.3e} (worst err / tol {ratio:.3f}) over {int(touched.sum())} channels")
    assert (err[touched] <= tol[touched]).all()
    assert err[touched].max() <= 1.01 * cases.CHAIN_ERROR
    np.testing.assert_array_equal(c32[st["per_pixel"] == 0], cases.target_of(s)[st["per_pixel"] == 0])


def test_the_recorded_chain_error_is_the_measured_one(scenes, restated):
    """tests/transparent_cases.py CHAIN_ERROR, of which the GPU test allows 4 x, is the worst |c32 - c64| over the cases' finite touched channels, within 1 %"""
    worst = 0.0
    for name, (depth, L, st, c32, c64) in restated.items():
        with np.errstate(all="ignore"):
            err = np.abs(c32.astype(np.float64) - c64)
        worst = max(worst, float(err[(st["per_pixel"] > 0)[..., None] & np.isfinite(c64)].max()))
    print(f"worst |c32 - c64| over the cases: {worst:.4e}")
    assert 0.99 * cases.CHAIN_ERROR <= worst <= 1.01 * cases.CHAIN_ERROR


MUTANTS = {   # mutant -> (the case that catches it, how the restatement is bent)
    "peeling by depth instead of order": ("order_abc", dict(layers=dict(by_depth=True))),
    "> for >= in the depth test": ("depth_edge", dict(layers=dict(strict=True))),
    "ADD for SUBTRACT in the alpha op": ("order_abc", dict(composite=dict(add_alpha=True))),
    "reversed order": ("mixed_modes", dict(layers=dict(reverse=True))),
    "a discarded fragment taking a layer": ("cutout_gltf", dict(layers=dict(discarded_take_a_layer=True))),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_each_mutant_of_the_restatement_is_caught_by_its_case(scenes, restated, mutant):
    name, how = MUTANTS[mutant]
    s = scenes[name]
    depth, L, st, c32, c64 = restated[name]
    bent, _ = tr.layers(s, depth, **how.get("layers", {}))
    got = tr.composite(bent, cases.shaders(s, depth)[0], cases.target_of(s), np.float32, **how.get("composite", {}))
    tol = cases.chain_tolerance(L, cases.shaders(s, depth)[1], cases.target_of(s), 4 * cases.CHAIN_ERROR)
    beyond = np.abs(got.astype(np.float64) - c64) > tol
    print(f"[{mutant}] {int(beyond.any(axis=-1).sum())} pixels of {name} beyond the end-to-end bound")
    assert beyond.any(axis=-1).sum() > 20, f"{name} does not catch: {mutant}"
