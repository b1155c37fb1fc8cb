"""CPU suite of the bloom path: ABI and layouts, the opt-in registration, the fp32 group-wise source-texel arithmetic and the conditions on the test
inputs, the vectorised restatement of tests/bloom_ref.py held against a literal scalar transliteration of the two shaders (tile, barrier, load_lds) and
against its float64 twin, closed forms, and the golden chain.  No GPU needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import bloom_ref as ref
from bloom_cases import CASES, FINITE_CASES, SHIPPED, make_dirt, make_main
from sailor_amd import _lib, host, runtime_binding

ROOT = Path(__file__).resolve().parents[1]
F = np.float32
SYMBOLS = ("sailor_hip_bloom_downscale", "sailor_hip_bloom_upscale", "sailor_hip_bloom", "sailor_hip_mip_chain_texels", "sailor_host_bloom_push_constants")


def test_abi_symbols_version_and_struct_layout():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    declared = set(re.findall(r"\b(sailor_(?:hip|host)_\w+)\s*\(", header))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.sailor_hip_version() >= 6
    assert C.sizeof(_lib.BloomParams) == 16
    assert [(n, getattr(_lib.BloomParams, n).offset) for n, _ in _lib.BloomParams._fields_] == [
        ("threshold", 0), ("knee", 4), ("bloomIntensity", 8), ("dirtIntensity", 12)]
    assert re.search(r"typedef struct SailorBloomParams \{\s*float threshold;\s*float knee;\s*float bloomIntensity;\s*float dirtIntensity;\s*\}", header)
    p = host.bloom_params()
    assert (p.threshold, F(p.knee), F(p.bloomIntensity), p.dirtIntensity) == (3.0, F(0.2), F(1.3), 5.0)   # DefaultRenderer.renderer:298-302
    assert host.bloom_params(knee=0.5).knee == 0.5
    assert _lib.BLOOM_SHIPPED == dict(threshold=SHIPPED["threshold"], knee=SHIPPED["knee"], bloomIntensity=SHIPPED["bloom_intensity"],
                                      dirtIntensity=SHIPPED["dirt_intensity"])


def test_push_constants_are_the_nodes_not_the_shader_comments():
    """BloomNode.cpp:93: .w = 0.25 * knee, a product (the shader's comment expects the curve of a quotient): restated"""
    got = host.bloom_push_constants(3.0, 0.2)
    t, k = F(3.0), F(0.2)
    assert got.dtype == F and got.tolist() == [t, t - k, F(2.0) * k, F(0.25) * k]
    assert np.array_equal(got, ref.push_constants(3.0, 0.2))
    assert _lib.load().sailor_host_bloom_push_constants(3.0, 0.2, None) == -1


def test_mip_chain_helper_matches_the_render_target_layout():
    for (w, h, levels) in [(3840, 2160, 8), (320, 200, 6), (270, 135, 5), (72, 40, 8), (1, 1, 1), (5, 1, 4)]:
        ext = ref.chain_extents(w, h, levels)
        assert host.mip_chain_extents(w, h, levels) == ext
        for l in range(levels + 1):
            assert host.mip_chain_texels(w, h, l) == sum(a * b for a, b in ext[:l])
    assert ref.chain_extents(3840, 2160, 8)[-1] == (30, 16) and ref.chain_extents(270, 135, 3)[1:] == [(135, 67), (67, 33)]
    assert host.mip_chain_texels(0, 4, 2) == 0 and host.mip_chain_texels(4, 4, -1) == 0 and host.mip_chain_texels(4, 4, 99) == 0


def test_bloom_is_opt_in_and_never_registered():
    rt = runtime_binding.load()
    assert hasattr(rt, "sailor_rt_enable_node") and hasattr(rt, "sailor_rt_set_color_target_chain")
    assert rt.sailor_rt_node_registered(b"Bloom") == 0
    assert rt.sailor_rt_enable_node(None, b"Bloom") == -1      # no runtime to opt in
    assert rt.sailor_rt_node_registered(b"Bloom") == 0
    assert rt.sailor_rt_node_registered(b"EyeAdaptation") == 1


def test_shipped_renderer_file_has_the_bloom_entry_between_render_scene_and_eye_adaptation():
    text = (ROOT / "tests" / "golden" / "DefaultRenderer.renderer").read_text()
    _, summary = runtime_binding.parse_renderer(text, 3840, 2160)
    nodes = summary[summary.index("nodes="):summary.index(";values=")]
    entry = "Bloom[]{vec4 bloomIntensity=1.3 0 0 0;vec4 dirtIntensity=5 0 0 0;vec4 knee=0.2 0 0 0;vec4 threshold=3 0 0 0;rt bloom=Main;}"
    assert entry in nodes, nodes
    assert nodes.rindex("RenderScene[") < nodes.index(entry) < nodes.index("EyeAdaptation[")
    assert "Main:3840x2160:R16G16B16A16_SFLOAT:8" in summary
    assert "g_lensDirtSampler" in summary[summary.index(";samplers="):]


# ---- the source-texel arithmetic -------------------------------------------------------------------------------------------------------------
def literal_tile_indices(read_dim: int, write_dim: int, group: int):
    """the ten source indices of one axis of one group's tile, as the shaders' loop computes them (scalar float32)"""
    texel = F(1.0) / F(write_dim)
    uv = (F(8 * group - 1) + F(0.5)) * texel
    return [int(F(read_dim) * (uv + F(slot) * texel)) for slot in range(10)]


@pytest.mark.parametrize("read_dim,write_dim", [(2160, 1080), (200, 100), (320, 160), (135, 67), (270, 135), (128, 64), (96, 48), (25, 12), (3, 1), (1, 1),
                                                 (100, 200), (67, 135), (12, 25), (1, 2)])
def test_indices_are_the_tile_slots_of_the_asking_group(read_dim, write_dim):
    got = ref.src_indices(read_dim, write_dim)
    for p in range(write_dim):
        tile = literal_tile_indices(read_dim, write_dim, p >> 3)
        assert [int(got[d, p]) for d in range(3)] == [tile[(p & 7) + d] for d in range(3)], p


def test_the_two_effects_of_the_fp32_arithmetic_and_where_they_show():
    """the figures of the 4K rows, and which of the test sizes show taps that are not 2 p + 1 and neighbours that depend on the asking group"""
    assert ref.index_effects(2160, 1080) == (828, 78)
    assert ref.index_effects(200, 100) == (73, 4)
    assert ref.index_effects(128, 64) == (0, 0) and ref.index_effects(96, 48) == (0, 0)
    c = CASES["c320x200"]
    assert (c.width, c.height) == (320, 200)
    nn, amb = ref.index_effects(c.height, c.height >> 1)
    assert nn > 0 and amb > 0, "a test size must show both effects"
    o = CASES["odd270x135"]
    assert ref.index_effects(o.width, o.width >> 1)[0] > 0 and ref.index_effects(o.width, o.width >> 1)[1] > 0
    p = CASES["pow2_128x96"]
    assert ref.index_effects(p.width, p.width >> 1) == (0, 0) and ref.index_effects(p.height, p.height >> 1) == (0, 0)
    assert len(FINITE_CASES) > 1, "128 x 96 shows neither effect and cannot be the only size"


def test_downscale_has_one_outside_texel_per_side_and_the_upscale_only_above():
    for r, w in [(200, 100), (320, 160), (135, 67), (128, 64)]:
        idx = ref.src_indices(r, w)
        assert idx.min() == -1 and (idx == -1).sum() == 1 and idx[0, 0] == -1
        assert idx.max() <= r + 1 and (idx >= r).sum() >= 1
    for r, w in [(100, 200), (160, 320), (67, 135), (64, 128)]:
        idx = ref.src_indices(r, w)
        assert idx.min() == 0, "the lower halo (about -0.25) truncates toward zero to texel 0"
        assert idx.max() == r and (idx == r).sum() == 1 and idx[2, w - 1] == r


def test_chains_have_an_odd_level():
    assert (135, 67) in ref.chain_extents(270, 135, CASES["odd270x135"].levels)
    assert (40, 25) in ref.chain_extents(320, 200, CASES["c320x200"].levels) and (20, 12) in ref.chain_extents(320, 200, CASES["c320x200"].levels)
    assert ref.chain_extents(72, 40, CASES["hostile72x40"].levels)[-1] == (1, 1)


@pytest.mark.parametrize("name", FINITE_CASES)
def test_thresholded_level_one_has_zero_and_non_zero_texels(name):
    c = CASES[name]
    main = make_main(c)
    (w1, h1) = ref.chain_extents(c.width, c.height, 2)[1]
    l1 = ref.downscale(main, w1, h1, ref.push_constants(c.threshold, c.knee), True)
    zero = float((l1[..., :3] == 0).all(axis=-1).mean())
    print(name, "zero share of level 1:", zero)
    assert np.isfinite(l1).all() and zero >= 0.05 and 1.0 - zero >= 0.05, zero
    knee_part = ref.downscale(main, w1, h1, ref.push_constants(c.threshold, c.knee), False)
    br = knee_part[..., :3].max(axis=-1)
    if name == "pow2_128x96":   # the wide knee: some texels sit on the quadratic part of the curve
        assert ((br > F(c.threshold - c.knee)) & (br < F(c.threshold + c.knee))).mean() > 0.02


# ---- the vectorised restatement against a literal scalar transliteration of the shaders ----------------------------------------------------------
def literal_dispatch(src, dst_w, dst_h, body):
    """one Dispatch of ceil(w / 8) x ceil(h / 8) groups of 8 x 8: fill the 10 x 10 tile (r, g, b only), barrier, then `body(load_lds, x, y)` per in-range thread"""
    RH, RW = src.shape[:2]
    out = {}
    for gy in range((dst_h + 7) // 8):
        for gx in range((dst_w + 7) // 8):
            tx, ty = literal_tile_indices(RW, dst_w, gx), literal_tile_indices(RH, dst_h, gy)
            tile = np.zeros((100, 3), F)
            for i in range(100):
                x, y = tx[i % 10], ty[i // 10]
                if 0 <= x < RW and 0 <= y < RH:
                    tile[i] = src[y, x, :3]
            load = lambda idx: np.array([tile[idx, 0], tile[idx, 1], tile[idx, 2], F(1.0)], F)
            for ly in range(8):
                for lx in range(8):
                    x, y = gx * 8 + lx, gy * 8 + ly
                    if x < dst_w and y < dst_h:   # a store outside the image is dropped
                        out[(y, x)] = body(load, (lx + 1) + (ly + 1) * 10, x, y)
    res = np.zeros((dst_h, dst_w, 4), F)
    for (y, x), v in out.items():
        res[y, x] = v
    return res


def literal_downscale(src, dst_w, dst_h, th, use_threshold):
    def karis(c):
        luma = (c[0] * F(0.2126729) + c[1] * F(0.7151522)) + c[2] * F(0.0721750)
        return c / (F(1.0) + luma)

    def body(load, s, x, y):
        A, B, Cc = load(s - 11), load(s - 10), load(s - 9)
        Fm, G, H = load(s - 1), load(s), load(s + 1)
        K, L, M = load(s + 9), load(s + 10), load(s + 11)
        D = (A + B + G + Fm) * F(0.25)
        E = (B + Cc + H + G) * F(0.25)
        I = (Fm + G + L + K) * F(0.25)
        J = (G + H + M + L) * F(0.25)
        dx, dy = F(1.0 / 4.0) * F(0.5), F(1.0 / 4.0) * F(0.125)
        c = karis((D + E + I + J) * dx)
        c = c + karis((A + B + G + Fm) * dy)
        c = c + karis((B + Cc + H + G) * dy)
        c = c + karis((Fm + G + L + K) * dy)
        c = c + karis((G + H + M + L) * dy)
        if use_threshold:
            br = max(c[0], max(c[1], c[2]))
            rq = min(max(br - th[1], F(0.0)), th[2])
            rq = th[3] * rq * rq
            c = c * (max(rq, br - th[0]) / max(br, F(1.0e-4)))
        return c
    return literal_dispatch(src, dst_w, dst_h, body)


def literal_upscale(src, dst, mip_level, bi, di, dirt):
    H, W = dst.shape[:2]
    tex = None
    if mip_level == 1 and dirt is not None:
        u = (np.arange(W).astype(F) + F(0.5)) * (F(1.0) / F(W))
        v = (np.arange(H).astype(F) + F(0.5)) * (F(1.0) / F(H))
        tex = ref.sample_repeat(dirt, u, v)

    def body(load, s, x, y):
        acc = load(s - 11)
        acc = acc + load(s - 10) * F(2.0)
        acc = acc + load(s - 9)
        acc = acc + load(s - 1) * F(2.0)
        acc = acc + load(s) * F(4.0)
        acc = acc + load(s + 1) * F(2.0)
        acc = acc + load(s + 9)
        acc = acc + load(s + 10) * F(2.0)
        acc = acc + load(s + 11)
        bloom = acc * F(1.0 / 16.0)
        out = dst[y, x] + bloom * F(bi)
        if tex is not None:
            out = out + tex[y, x] * F(di) * bloom * F(bi)
        return out
    return literal_dispatch(src, W, H, body)


@pytest.mark.parametrize("w,h", [(40, 24), (27, 13), (50, 25)])
def test_vectorised_restatement_equals_the_literal_shaders(w, h):
    rng = np.random.default_rng(w * 100 + h)
    main = np.ones((h, w, 4), F)
    main[..., :3] = np.exp(rng.normal(0.0, 2.0, (h, w, 3))).astype(F)
    main[..., 2] *= F(30.0)
    main[:, :w // 2, :3] *= F(0.02)   # a dim half that stays under the threshold
    dirt = make_dirt(seed=3, width=7, height=5)
    th = ref.push_constants(3.0, 0.2)
    (w1, h1), (w2, h2) = ref.chain_extents(w, h, 3)[1:]
    with np.errstate(all="ignore"):
        for use in (True, False):
            a, b = ref.downscale(main, w1, h1, th, use), literal_downscale(main, w1, h1, th, use)
            assert ref.same_bits(a, b)[0], ("downscale", use, ref.same_bits(a, b)[1])
        l1 = ref.downscale(main, w1, h1, th, True)
        assert (l1[..., :3] != 0).any() and (l1[..., :3] == 0).all(axis=-1).any()
        l2 = ref.downscale(l1, w2, h2, th, False)
        for level, src, dst, d in ((2, l2, l1, dirt), (1, l1, main, dirt), (1, l1, main, None)):
            a, b = ref.upscale(src, dst, level, 1.3, 5.0, d), literal_upscale(src, dst, level, 1.3, 5.0, d)
            assert ref.same_bits(a, b)[0], ("upscale", level, d is None, ref.same_bits(a, b)[1])
        assert not np.array_equal(ref.upscale(l1, main, 1, 1.3, 5.0, dirt), ref.upscale(l1, main, 1, 1.3, 5.0, None)), "the dirt term changes level 0"
        assert np.array_equal(ref.upscale(l2, l1, 2, 1.3, 5.0, dirt), ref.upscale(l2, l1, 2, 1.3, 5.0, None)), "... and only at mip level 1"


def test_closed_form_of_a_uniform_image():
    """every tap (g, g, g, 1): c = 0.5 g / (1 + 0.5 g L) + 4 * 0.125 g / (1 + 0.125 g L), alpha the same with g = 1 upstairs; the upscale adds
    16 / 16 of the source times bloomIntensity to every channel, alpha included"""
    L = sum(ref.LUMA)
    g = 2.5
    src = np.full((32, 32, 4), g, F)
    src[..., 3] = 7.0   # the tile drops alpha
    out = ref.downscale(src, 16, 16, ref.push_constants(3.0, 0.2), False)
    want_rgb = 0.5 * g / (1 + 0.5 * g * L) + 4 * 0.125 * g / (1 + 0.125 * g * L)
    want_a = 0.5 / (1 + 0.5 * g * L) + 4 * 0.125 / (1 + 0.125 * g * L)
    inner = out[2:-2, 2:-2]
    assert np.allclose(inner[..., :3], want_rgb, rtol=1e-6) and np.allclose(inner[..., 3], want_a, rtol=1e-6)
    assert out[0, 0, 0] < inner[0, 0, 0], "the texels in front of the image are zero"
    dst = np.full((32, 32, 4), 0.25, F)
    up = ref.upscale(np.full((16, 16, 4), g, F), dst, 2, 1.3, 5.0, None)
    assert np.allclose(up[2:-2, 2:-2, :3], 0.25 + 1.3 * g, rtol=1e-6) and np.allclose(up[2:-2, 2:-2, 3], 0.25 + 1.3, rtol=1e-6)


def test_threshold_curve_values():
    """quadratic_threshold on one pixel: under t - knee -> 0; over t + knee -> c (br - t) / br; in the knee -> the node's curve with .w = 0.25 knee"""
    th = ref.push_constants(3.0, 0.2, np.float64)

    def factor(br):
        rq = min(max(br - th[1], 0.0), th[2])
        return max(th[3] * rq * rq, br - th[0]) / max(br, 1e-4)
    assert factor(2.0) == 0.0 and factor(2.79) == 0.0
    assert factor(10.0) == pytest.approx(0.7)
    assert factor(3.0) == pytest.approx(0.05 * 0.2 * 0.2 / 3.0)   # 0.25 knee * (knee)^2 / br: the product form, not 0.25 / knee
    assert factor(2.9) > 0.0


def test_hostile_texels_go_through_the_whole_pyramid():
    c = CASES["hostile72x40"]
    main = make_main(c)
    assert not np.isfinite(main).all()
    lv = ref.bloom_chain(main, c.levels, dirt=make_dirt(), **c.params())
    assert len(lv) == c.levels and lv[-1].shape == (1, 1, 4)
    assert np.isnan(lv[0]).any() and np.isfinite(lv[0]).mean() > 0.5, "hostile texels spread through the pyramid, but not everywhere"


# ---- fp32 against float64 -------------------------------------------------------------------------------------------------------------------------
# Largest |fp32 - float64| per level of the whole chain (index = level), relative to that level's largest float64 magnitude, measured on the three
# finite cases with the seeded dirt texture (float64 values, fp32 indices; rounded up to three digits):
#   c320x200    1.26e-6  2.21e-7  1.74e-7  1.78e-7  1.37e-7  1.69e-7
#   odd270x135  7.26e-7  1.89e-7  1.49e-7  1.35e-7  1.15e-7
#   pow2_128x96 1.83e-7  1.38e-7  1.26e-7  1.32e-7  1.32e-7
# Level 0 is the largest where the dirt product of 5 x bloom comes on top of the sum of all levels.  The bound is 4 x the largest of them per level.
MEASURED_REL_ERR = [1.26e-6, 2.22e-7, 1.75e-7, 1.79e-7, 1.38e-7, 1.70e-7]


@pytest.mark.parametrize("name", FINITE_CASES)
def test_fp32_restatement_against_float64(name):
    c = CASES[name]
    main, dirt = make_main(c), make_dirt()
    a = ref.bloom_chain(main, c.levels, dirt=dirt, **c.params())
    b = ref.bloom_chain(main, c.levels, dirt=dirt, dtype=np.float64, **c.params())
    figures = []
    for level, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == F and y.dtype == np.float64 and np.isfinite(y).all()
        scale = np.abs(y).max()
        err = np.abs(x.astype(np.float64) - y).max() / scale
        figures.append(float(err))
    print(name, "max |fp32 - float64| / level max, per level:", ["%.3g" % e for e in figures])
    for level, err in enumerate(figures):
        assert err <= 4.0 * MEASURED_REL_ERR[level], (name, level, err)


def test_golden_chain_of_the_tiny_image():
    gold = np.load(ROOT / "tests" / "golden" / "tiny_bloom.npz")
    main, dirt = gold["main"], gold["dirt"]
    assert main.shape == (24, 40, 4) and dirt.shape == (3, 5, 4) and main.dtype == F
    lv = ref.bloom_chain(main, 3, dirt=dirt, **SHIPPED)
    for l, v in enumerate(lv):
        np.testing.assert_array_equal(np.ascontiguousarray(v).view(np.uint32), gold[f"level{l}_bits"])
    assert not np.array_equal(lv[0], main)
