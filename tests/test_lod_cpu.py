"""Mip-mapped material textures without a GPU: tests/lod_ref.py (the float32 restatement the kernels are held to) against its float64 twin of the chain, the
known answers of the level selection, the restatement with one-level tables against surface_ref, masked_ref and gltf_ref bit for bit, what every case of
tests/lod_cases.py was built to reach, and the C-ABI's layout, version, symbols and host helpers."""
import ctypes as C
import math

import numpy as np
import pytest

import gltf_cases
import gltf_ref
import lod_cases as cases
import lod_ref
import masked_cases
import masked_ref
import surface_cases
import surface_ref
from sailor_amd import _lib, host

f32, f64 = np.float32, np.float64
SYMBOLS = ("sailor_hip_texture_generate_mips", "sailor_hip_texture_mip_levels", "sailor_host_srgb_encode_table", "sailor_hip_surface_resolve_lod",
           "sailor_hip_surface_draw_lod", "sailor_hip_surface_draw_indirect_lod")
# max |lambda32 - lambda64| over every fragment that blends two levels in the cases of tests/lod_cases.py and in aligned_quad(3), measured on the restatement
# (2.58e-7 in the cases, 2.3e-8 in the quad; DESIGN.md section 4 records it): the known-answer tolerance is 4 x this
LAMBDA_ERR = 2.6e-7
COLOURS = [cases.unorm(c).astype(f64)[:3] for c in cases.LEVEL_COLOURS]


# ---- 1. the chain against its float64 twin -----------------------------------------------------------------------------------------------------------------
def test_the_chain_is_its_float64_twin_up_to_exact_ties():
    """every byte of every level, the seven extents, sRGB and UNORM, seeds 0-19: at most 1 from the float64 twin's, and a byte that differs is one whose
    float64 value lies within 1e-6 of the boundary spacing from a rounding boundary.  Measured: 4 521 of 233 440 bytes differ, the farthest 8.3e-7 of a spacing
    from its boundary (UNORM means of four bytes tie exactly in a quarter of the texels; the twin decides those by its own rounding)."""
    total = differing = 0
    worst = 0.0
    for seed in range(20):
        for (w, h) in cases.EXTENTS:
            for srgb in (False, True):
                level = cases.random_texture(w, h, 1000 * seed + 7 * w + h)
                for _ in range(lod_ref.full_levels(w, h) - 1):
                    got = lod_ref.next_level(level, srgb)
                    twin, margin = lod_ref.next_level64(level, srgb)
                    d = got.astype(np.int64) - twin.astype(np.int64)
                    assert np.abs(d).max() <= 1, (seed, w, h, srgb)
                    total, differing = total + d.size, differing + int((d != 0).sum())
                    if (d != 0).any():
                        worst = max(worst, float(margin[d != 0].max()))
                    level = got
                assert level.shape == (1, 1, 4)
    print(f"[chain] {differing} of {total} bytes differ from the float64 twin; the farthest lies {worst:.3g} of a boundary spacing from its boundary")
    assert total > 200000 and worst <= 1e-6


def test_chain_layout_and_even_extents_are_the_2x2_mean():
    for (w, h) in cases.EXTENTS:
        chain = lod_ref.build_chain(cases.random_texture(w, h, 3), True)
        assert len(chain) == lod_ref.full_levels(w, h) == int(math.floor(math.log2(max(w, h)))) + 1
        assert [c.shape[:2] for c in chain] == [(max(h >> l, 1), max(w >> l, 1)) for l in range(len(chain))]
        assert lod_ref.flat_chain(chain).size == lod_ref.chain_offset(w, h, len(chain))
    img = cases.random_texture(8, 8, 5)
    got = lod_ref.next_level(img, False).astype(f64)
    mean = img.astype(f64).reshape(4, 2, 4, 2, 4).mean(axis=(1, 3))
    assert np.abs(got - mean).max() <= 0.5 + 1e-9        # the rounded 2 x 2 mean
    assert (lod_ref.next_level(np.full((4, 4, 4), 77, np.uint8), True) == 77).all() and (lod_ref.next_level(np.full((5, 3, 4), 200, np.uint8), False) == 200).all()


# ---- 2. known answers --------------------------------------------------------------------------------------------------------------------------------------
def check_known_answers(render):
    """the known answers of the level selection on `render` (the restatement here, the device in tests/test_lod_gpu.py): hand-made chains whose level l is the
    constant COLOURS[l], a screen-aligned quad"""
    for k in range(7):                                   # 2^k texels per pixel: level k (the rounding of the interpolated texcoord moves lambda by under 1e-5)
        p2 = render(cases.aligned_quad(2 ** k))["planes"][2][..., :3]
        assert np.abs(p2 - COLOURS[k]).max() <= 1e-4, k
    p2 = render(cases.anisotropic())["planes"][2][..., :3]         # 8 texels per pixel in u, 1 in v: the larger axis decides
    assert np.abs(p2 - COLOURS[3]).max() <= 1e-4
    s = cases.aligned_quad(0.5)                                     # magnification: level 0 alone, the one-level fetch bit for bit
    p2 = render(s)["planes"][2][..., :3]
    assert np.abs(p2 - COLOURS[0]).max() <= 1e-4 and np.array_equal(p2.view(np.uint32), lod_ref.render(cases.one_level(s))["planes"][2][..., :3].view(np.uint32))
    # 3 texels per pixel: levels 1 and 2 under delta = log2(3) - 1.  Their colours are (0, 1, 0) and (0, 0, 1), so P2.g = 1 - delta and P2.b = delta
    s = cases.aligned_quad(3)
    want = lod_ref.render(s)
    p2 = render(s)["planes"][2]
    seen = 0
    for (at, ii, jj, lam32, lam64) in want["stats"]["lambdas"]:
        if at != 0:
            continue
        assert np.abs(lam64 - math.log2(3)).max() < 1e-5
        assert np.abs(lam32.astype(f64) - lam64).max() <= LAMBDA_ERR
        delta = lam64 - 1.0
        assert np.abs(p2[jj, ii, 2] - delta).max() <= 4 * LAMBDA_ERR and np.abs(p2[jj, ii, 1] - (1.0 - delta)).max() <= 4 * LAMBDA_ERR and (p2[jj, ii, 0] == 0).all()
        seen += len(ii)
    assert seen == s["W"] * s["H"]


def test_known_answers_in_the_restatement():
    check_known_answers(lod_ref.render)
    scenes = list(cases.all_scenes().values()) + [cases.aligned_quad(3)]
    worst = max(float(np.abs(l32.astype(f64) - l64).max()) for s in scenes for (_, _, _, l32, l64) in lod_ref.render(s)["stats"]["lambdas"])
    print(f"[lambda] max |lambda32 - lambda64| over every blended fragment of the cases and of aligned_quad(3): {worst:.3g}")
    assert LAMBDA_ERR / 2 < worst <= LAMBDA_ERR        # the constant is the measurement, not a wish


def test_level_selection_edges():
    one = lambda r: [np.array([q], f32) for q in (r, 0, 0, 0)]       # dudx alone, in texcoord units
    sel = lambda w, h, n, dudx: tuple(x[0] for x in lod_ref.select_levels(w, h, n, one(dudx)))
    assert sel(64, 64, 7, 1 / 64) == (0, 0, False) and sel(64, 64, 7, 0.0) == (0, 0, False) and sel(64, 64, 7, np.nan) == (0, 0, False)
    assert sel(64, 64, 7, np.inf) == (6, 0, False) and sel(64, 64, 7, 1.0) == (6, 0, False) and sel(64, 64, 7, 100.0) == (6, 0, False)
    assert sel(64, 64, 7, 2 / 64) == (1, 0, True) and sel(64, 64, 7, 32 / 64)[0] == 5 and sel(64, 64, 3, 4 / 64) == (2, 0, False)
    assert sel(64, 64, 1, 1.0) == (0, 0, False)
    hi, delta, blend = sel(16, 4, 5, 3 / 16)
    assert hi == 1 and blend and abs(float(delta) - (math.log2(3) - 1)) < 1e-6
    # the larger of the two axes, each with the descriptor's own extents: dvdy in a 16 x 4 texture counts a quarter of dudx
    d = [np.array([q], f32) for q in (2 / 16, 0, 0, 4 / 4)]
    assert lod_ref.select_levels(16, 4, 5, d)[0][0] == 2
    assert [lod_ref.level_count(17, 9, f) for f in (0, 1, 3, 5, 99)] == [1, 1, 3, 5, 5] and lod_ref.level_count(1, 1, 99) == 1


# ---- 3. no behaviour change --------------------------------------------------------------------------------------------------------------------------------
def same(got, want, keys, what):
    for k in keys:
        assert surface_ref.same_bits_or_class(np.asarray(got[k]).astype(f32) if got[k].dtype == bool else got[k],
                                              np.asarray(want[k]).astype(f32) if want[k].dtype == bool else want[k]).all(), (what, k)
    np.testing.assert_array_equal(got["keys"], want["keys"], err_msg=what)
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), err_msg=what)


def test_one_level_tables_are_surface_ref_masked_ref_and_gltf_ref_bit_for_bit():
    n = 0
    for name, (build, _) in surface_cases.CASES.items():
        s = build()
        same(lod_ref.render(s), surface_ref.render(s), ("planes", "covered"), name)
        n += 1
    for seed in range(0, surface_cases.NUM_SOUPS, 4):
        s = surface_cases.random_soup(seed)
        same(lod_ref.render(s), surface_ref.render(s), ("planes", "covered"), f"soup {seed}")
    for name, s in masked_cases.all_scenes().items():
        same(lod_ref.render(s), masked_ref.render(s), ("planes", "covered"), name)
        n += 1
    for name, s in gltf_cases.all_scenes().items():
        same(lod_ref.render(s), gltf_ref.render(s), ("planes", "covered", "emissive", "ao_out", "gltf", "cutout"), name)
        n += 1
    for name, (build, _) in cases.CASES.items():          # and the cases here with their chains taken away
        s = cases.one_level(build())
        same(lod_ref.render(s), gltf_ref.render(s), ("planes", "covered", "emissive", "ao_out"), name)
    assert n > 60


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered():
    return {name: (s, lod_ref.render(s)) for name, s in cases.all_scenes().items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_reaches_what_it_was_built_for(rendered, name):
    s, r = rendered[name]
    assert s["W"] <= 48 and s["H"] <= 32
    assert cases.CASES[name][1](r, s), {k: v for k, v in r["stats"].items() if k not in ("alpha", "threshold", "lambdas")}


def test_the_cases_use_the_seven_extents():
    seen = {(t.shape[1], t.shape[0]) for s in cases.all_scenes().values() for t in s["textures"]}
    assert set(cases.EXTENTS) <= seen, set(cases.EXTENTS) - seen


def test_chains_change_the_picture_and_the_discard(rendered):
    for name in ("receding_ground", "mixed_pass", "cutout_per_level"):
        s, r = rendered[name]
        flat = lod_ref.render(cases.one_level(s))
        assert not surface_ref.same_bits_or_class(r["planes"], flat["planes"]).all(), name
    s, r = rendered["cutout_per_level"]
    assert (r["covered"] != lod_ref.render(cases.one_level(s))["covered"]).sum() > 20       # the level decides who is discarded


def test_every_cutout_owned_pixel_holds_the_alpha_that_was_tested(rendered):
    s, r = rendered["cutout_per_level"]
    own = r["cutout"] & r["covered"]
    alpha, threshold = r["stats"]["alpha"], r["stats"]["threshold"]
    np.testing.assert_array_equal(r["planes"][0][own][:, 3].view(np.uint32), alpha[own].view(np.uint32))
    assert (alpha[own] >= threshold[own]).all() and set(np.unique(threshold[own])) == {f32(0.5), f32(0.3)}


def test_bands_need_no_neighbour_rows(rendered):
    for name in cases.BAND_CASES:
        s, whole = rendered[name]
        for world in (2, 3):
            parts = []
            for rank in reversed(range(world)):
                band = host.band_for_rank(s["W"], s["H"], rank, world)
                if band.fbRowCount:
                    parts.append(lod_ref.render(s, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)))
            np.testing.assert_array_equal(np.concatenate([p["keys"] for p in parts]), whole["keys"])
            assert surface_ref.same_bits_or_class(np.concatenate([p["planes"] for p in parts], axis=1), whole["planes"]).all(), (name, world)


# ---- 4. the C-ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_layout_version_and_symbols():
    lib = _lib.load()
    assert C.sizeof(_lib.TextureDesc) == 24 and _lib.TextureDesc.levels.offset == 20 and _lib.TextureDesc.flags.offset == 16 and _lib.TextureDesc.levels.size == 4
    assert lib.sailor_hip_version() >= 11
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def test_host_helpers():
    for (w, h) in cases.EXTENTS + ((32768, 1), (3, 32768), (1000, 513), (2, 2)):
        n = host.texture_mip_levels(w, h)
        assert n == lod_ref.full_levels(w, h) == int(math.floor(math.log2(max(w, h)))) + 1, (w, h)
        for l in range(n + 1):
            assert host.mip_chain_texels(w, h, l) == lod_ref.chain_offset(w, h, l)
    assert [host.texture_mip_levels(*e) for e in ((0, 4), (4, 0), (-1, 4), (32769, 1), (1, 32769))] == [0] * 5
    enc = host.srgb_encode_table()
    assert enc.dtype == np.float32 and np.array_equal(enc.view(np.uint32), lod_ref.encode_table().view(np.uint32)) and (np.diff(enc) > 0).all()
    dec = host.srgb_table()
    assert (dec[:-1] < enc).all() and (enc < dec[1:]).all()           # every byte decodes strictly between its two boundaries: encode(decode(b)) == b
    assert np.array_equal(np.searchsorted(enc, dec, side="right"), np.arange(256))
    assert _lib.load().sailor_host_srgb_encode_table(None) == -1
