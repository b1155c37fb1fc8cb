"""CPU suite of the EyeAdaptation node (no GPU): the fp32 restatement the kernels are held against bit for bit (tests/eye_adaptation_ref.py)
against the float64 one, known answers and edge cases, the host constants, the C-ABI's new symbols and the stored fixture."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import eye_adaptation_ref as ref
from eye_adaptation_ref import Ref32, Ref64
from sailor_amd import _lib, host

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def log_uniform_pixels(n, seed=20251016):
    """n pixels, each channel log-uniform in [2^-12, 2^7]"""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(-12.0, 7.0, (n, 3))).astype(f32)


# ---------------------------------------------------------------------------------------------------------------
# fp32 restatement against float64
# ---------------------------------------------------------------------------------------------------------------
def test_fp32_bins_differ_from_float64_only_next_to_a_bin_edge():
    """2^20 log-uniform pixels: at most 1e-4 of them in another bin, none by more than one (the restatement itself: 9 of 1 048 576)"""
    rgb = log_uniform_pixels(1 << 20)
    d = Ref32.bins(rgb).astype(np.int64) - Ref64.bins(rgb).astype(np.int64)
    differ = int((d != 0).sum())
    print(f"bins: {differ} of {d.size} differ, largest step {int(np.abs(d).max())}")
    assert differ <= 1e-4 * d.size
    assert np.abs(d).max() <= 1


def test_fp32_adapted_luminance_matches_float64_from_the_same_counts():
    """relative difference <= 2^-12: the reference keeps the value in R16_SFLOAT (EyeAdaptationNode.cpp:91), half a half-precision ulp"""
    rgb = log_uniform_pixels(1 << 20).reshape(1024, 1024, 3)
    counts = Ref32.histogram(rgb)
    for last, dt in ((0.5, 1.0 / 60.0), (0.01, 0.25), (20.0, 1.0 / 144.0), (0.5, 10.0)):
        k32, k64 = Ref32.constants(1024, 1024, dt), Ref64.constants(1024, 1024, dt)
        a = float(Ref32.average(counts, last, k32[0], k32[2], k32[3], k32[4]))
        b = Ref64.average(counts, last, k64[0], k64[2], k64[3], k64[4])
        print(f"adapted luminance last={last} dt={dt:.4f}: fp32 {a!r} float64 {b!r} rel {abs(a - b) / abs(b):.3e}")
        assert abs(a - b) <= 2.0 ** -12 * abs(b)


@pytest.mark.parametrize("ops", ref.OPERATOR_SETS)
def test_fp32_tonemap_matches_float64(ops):
    """per finite pixel |d| <= 2^-11 max(1, largest |channel| of the float64 result): half-precision spacing at display scale"""
    rgb = log_uniform_pixels(1 << 20)
    ch = np.random.default_rng(7).integers(0, 3, len(rgb) // 8)
    rgb[::8][np.arange(len(ch)), ch] *= f32(1e-6)  # one channel of an eighth of the pixels
    img = np.concatenate([rgb, np.ones((len(rgb), 1), f32)], axis=1).reshape(1024, 1024, 4)
    for avg in (0.01, 0.5, 20.0):
        a, b = Ref32.tonemap(img, avg, ops), Ref64.tonemap(img, avg, ops)
        finite = np.isfinite(b).all(-1)
        assert finite.all() and np.isfinite(a).all()
        err = np.abs(a.astype(np.float64) - b).max(-1)
        tol = 2.0 ** -11 * np.maximum(1.0, np.abs(b).max(-1))
        print(f"tonemap ops={ops} avg={avg}: worst |d| {err.max():.3e}, worst |d| / tol {(err / tol).max():.3e}")
        assert (err <= tol).all()
        assert np.array_equal(a[..., 3], img[..., 3])


# ---------------------------------------------------------------------------------------------------------------
# known answers and edge cases
# ---------------------------------------------------------------------------------------------------------------
def constant_image(h, w, value):
    img = np.empty((h, w, 4), f32)
    img[..., :3] = f32(value)  # r = g = b = v: luminance v (0.2125 + 0.7154 + 0.0721 = 1)
    img[..., 3] = 1
    return img


@pytest.mark.parametrize("lum,expected_bin", [(1.0, 170), (0.3, 133), (2.0 ** -8 * 1.5, 13), (17.0, 255), (1000.0, 255), (0.004, 0)])
def test_a_constant_image_lands_in_one_closed_form_bin(lum, expected_bin):
    # bin = uint(clamp((log2 L + 8) / 12, 0, 1) 254 + 1): L = 1 -> 170.33, L = 0.3 -> 133.57, L = 1.5 2^-8 -> 13.38, L > 16 -> 255
    img = constant_image(32, 48, lum)
    for R in (Ref32, Ref64):
        counts = R.histogram(img)
        assert counts[expected_bin] == 32 * 48 and counts.sum() == 32 * 48, (R.__name__, np.nonzero(counts))
    if expected_bin:
        k = Ref32.constants(48, 32, 1.0)
        adapted = Ref32.average(Ref32.histogram(img), 0.5, k[0], k[2], k[3], f32(1.0))  # timeCoeff = 1: the frame's own average
        assert float(adapted) == pytest.approx(2.0 ** ((expected_bin - 1) / 254.0 * 12.0 - 8.0), rel=2.0 ** -12)


def test_all_black_takes_the_minus_one_branch_and_zero_time_coeff_keeps_the_value():
    img = constant_image(16, 16, 0.0)
    counts = Ref32.histogram(img)
    assert counts[0] == 256 and counts.sum() == 256
    k = Ref32.constants(16, 16, 1.0)
    # sum = 0, denominator max(256 - 256, 1) = 1: weightedLogAverage = -1 -> exp2(-1 / 254 * 12 - 8)
    for R, kk in ((Ref32, k), (Ref64, Ref64.constants(16, 16, 1.0))):
        assert float(R.average(counts, 0.5, kk[0], kk[2], kk[3], 1.0)) == pytest.approx(2.0 ** (-12.0 / 254.0 - 8.0), rel=2.0 ** -12)
    assert Ref32.average(counts, 0.37, k[0], k[2], k[3], f32(0.0)) == f32(0.37)
    assert Ref32.constants(16, 16, 0.0)[4] == 0.0


def test_a_ragged_image_counts_whole_groups_and_divides_by_every_pixel():
    """100 x 52: the dispatch is (100 / 16, 52 / 16) = (6, 3) groups -> 96 x 48 pixels counted; numPixels stays 5 200"""
    img = constant_image(52, 100, 1.0)
    img[48:, :, :3] = 1000.0  # the uncounted remainder would land in bin 255
    img[:, 96:, :3] = 1000.0
    for R in (Ref32, Ref64):
        counts = R.histogram(img)
        assert counts[170] == 96 * 48 and counts.sum() == 96 * 48
        k = R.constants(100, 52, 1.0)
        assert float(k[3]) == 5200.0
        wla = 96 * 48 * 170 / 5200.0 - 1.0
        assert float(R.average(counts, 0.5, k[0], k[2], k[3], 1.0)) == pytest.approx(2.0 ** (wla / 254.0 * 12.0 - 8.0), rel=2.0 ** -12)


def test_the_weighted_sum_wraps_at_8k():
    """7680 x 4320 pixels in bin 255: 33 177 600 x 255 = 8 460 288 000 = 2^32 + 4 165 320 704"""
    counts = np.zeros(256, np.uint32)
    counts[255] = 7680 * 4320
    assert int(ref.weighted_sum_u32(counts)) == 7680 * 4320 * 255 - 2 ** 32 == 4165320704
    k = Ref32.constants(7680, 4320, 1.0)
    wla = 4165320704 / (7680 * 4320) - 1.0  # 124.5..., not 254
    for R, kk in ((Ref32, k), (Ref64, Ref64.constants(7680, 4320, 1.0))):
        assert float(R.average(counts, 0.5, kk[0], kk[2], kk[3], 1.0)) == pytest.approx(2.0 ** (wla / 254.0 * 12.0 - 8.0), rel=2.0 ** -12)
    spread = np.full(256, 7680 * 4320 // 256, np.uint32)
    assert int(ref.weighted_sum_u32(spread)) == (7680 * 4320 // 256 * (255 * 256 // 2)) % 2 ** 32


def hostile_image():
    """16 x 16: NaN, +-inf, negatives, exact black and a one-bin constant"""
    img = constant_image(16, 16, 0.3)
    img[0, 0, :3] = np.nan
    img[0, 1, :3] = np.inf
    img[0, 2, :3] = -np.inf
    img[0, 3, :3] = -3.0
    img[0, 4, :3] = 0.0
    img[0, 5, :3] = (np.inf, -np.inf, 1.0)  # inf - inf: NaN luminance
    img[0, 6, :3] = 3.0e38                   # finite, far above the range
    img[0, 7, :3] = (-1.0, 2.0, 0.0)         # a negative channel, positive luminance
    img[0, 8, :3] = 1.0e-30
    return img


def test_nan_inf_and_negative_luminance_land_where_the_rules_say():
    img = hostile_image()
    for R in (Ref32, Ref64):
        b = R.bins(img[0, :9, :3])
        assert list(b[:7]) == [0, 255, 0, 0, 0, 0, 255] and b[8] == 0 and 1 <= b[7] <= 255, (R.__name__, b)
        counts = R.histogram(img)
        assert counts.sum() == 256 and counts[133] == 256 - 9
    # the tone map keeps the classes: NaN in, NaN out; black under LUMINANCE is NaN (Formats.glsl:18), without it 0
    for ops in ref.OPERATOR_SETS:
        a, b = Ref32.tonemap(img, 0.5, ops), Ref64.tonemap(img, 0.5, ops)
        assert np.isnan(a[0, 0, :3]).all() and np.isnan(b[0, 0, :3]).all()
        black = a[0, 4, :3]
        assert np.isnan(black).all() if ops & ref.LUMINANCE else np.isfinite(black).all()
        keep = np.ones((16, 16), bool)
        keep[0, 6] = False  # 3e38 overflows in fp32 only
        assert (np.isfinite(a) == np.isfinite(b))[keep].all() and (np.isnan(a) == np.isnan(b))[keep].all()


def test_the_fixed_log2_and_exp2_are_accurate():
    x = np.exp2(np.linspace(-7.7, 20.0, 1 << 20)).astype(f32)
    assert np.abs(ref.canonical_log2f(x).astype(np.float64) - np.log2(x.astype(np.float64))).max() <= 1.0e-6
    e = np.linspace(-30.0, 30.0, 1 << 20).astype(f32)
    assert np.abs(ref.canonical_exp2f(e).astype(np.float64) / np.exp2(e.astype(np.float64)) - 1.0).max() <= 2.0 ** -22
    assert ref.canonical_exp2f(f32(3.0)) == 8.0 and ref.canonical_exp2f(f32(-8.0)) == 2.0 ** -8 and np.isnan(ref.canonical_exp2f(f32(np.nan)))
    assert ref.canonical_log2f(f32(1.0)) == 0.0 and ref.canonical_log2f(f32(0.25)) == -2.0


# ---------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,dt", [((3840, 2160), 1.0 / 60.0), ((7680, 4320), 0.004), ((100, 52), 0.25), ((128, 96), 0.0), ((1280, 720), 30.0)])
def test_host_constants_match_the_restatement(size, dt):
    c = host.eye_adaptation_constants(size[0], size[1], dt)
    k = Ref32.constants(size[0], size[1], dt)
    got = np.array([c.minLog2Luminance, c.invLog2LuminanceRange, c.log2LuminanceRange, c.numPixels], f32)
    assert np.array_equal(got.view(np.uint32), np.array(k[:4], f32).view(np.uint32))
    # timeCoeff goes through the host's exp2f: within one ulp
    assert abs(f32(c.timeCoeff) - k[4]) <= np.spacing(k[4]), (c.timeCoeff, k[4])
    assert 0.0 <= c.timeCoeff <= 1.0


def test_host_constants_refuse_bad_arguments():
    lib = _lib.load()
    c = _lib.EyeAdaptationConstants()
    assert lib.sailor_host_eye_adaptation_constants(0, 16, 0.1, C.byref(c)) == -1
    assert lib.sailor_host_eye_adaptation_constants(16, 16, 0.1, None) == -1


def test_the_abi_declares_and_exports_the_eye_adaptation_symbols():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    declared = set(re.findall(r"SAILOR_HIP_API\s+[\w\s\*]+?\b(sailor_\w+)\s*\(", header))
    wanted = {"sailor_hip_eye_adaptation_state_size", "sailor_hip_eye_adaptation_reset", "sailor_hip_eye_adaptation_state_views",
              "sailor_hip_luminance_histogram", "sailor_hip_average_luminance", "sailor_hip_tonemap", "sailor_hip_eye_adaptation",
              "sailor_host_eye_adaptation_constants"}
    assert wanted <= declared and wanted <= set(_lib.SIGNATURES)
    lib = C.CDLL(str(_lib.LIB_PATH))
    assert all(hasattr(lib, n) for n in wanted)
    assert _lib.load().sailor_hip_version() >= 3
    assert _lib.load().sailor_hip_eye_adaptation_state_size() >= 257 * 4
    assert C.sizeof(_lib.EyeAdaptationConstants) == 20
    for name, value in re.findall(r"#define SAILOR_TONEMAP_([A-Z0-9]+) (\d+)u", header):
        assert _lib.TONEMAP_DEFINES[name] == int(value)
    assert _lib.tonemap_flags("UNCHARTED2 LUMINANCE") == 6 and _lib.tonemap_flags("") == 0
    with pytest.raises(ValueError):
        _lib.tonemap_flags("REINHARD")


def test_device_entry_points_refuse_bad_arguments_without_a_context():
    lib = _lib.load()
    c = host.eye_adaptation_constants(16, 16, 0.1)
    band = host.band_whole_frame(16, 16)
    wp = (C.c_float * 4)(1.4, 1.5, 1.4, 0)
    assert lib.sailor_hip_luminance_histogram(None, 16, 16, 16, C.byref(band), C.byref(c), 16) == -1
    assert lib.sailor_hip_average_luminance(None, C.byref(c), 16) == -1
    assert lib.sailor_hip_tonemap(None, 16, 16, 16, 16, C.byref(band), 6, wp, 1.0, 16) == -1
    assert lib.sailor_hip_eye_adaptation(None, 16, 16, 16, 16, C.byref(c), 6, wp, 1.0, 16) == -1
    assert lib.sailor_hip_eye_adaptation_reset(None, 16, 0.5) == -1
    assert lib.sailor_hip_eye_adaptation_state_views(None, None, None) == -1 and lib.sailor_hip_eye_adaptation_state_views(8, None, None) == -1


def test_the_renderer_description_still_parses_to_the_same_counts():
    from sailor_amd import runtime_binding
    from test_host_cpu import RENDERER_TEXT
    n, summary = runtime_binding.parse_renderer(RENDERER_TEXT, 1280, 720)
    assert n == 6 and "Bloom[PostFx]" in summary


def test_the_stored_fixture_is_the_restatements():
    g = np.load(ROOT / "tests" / "golden" / "tiny_tonemap.npz")
    rad = g["radiance"]
    assert rad.dtype == f32 and np.array_equal(rad, np.load(ROOT / "tests" / "golden" / "tiny.npz")["radiance"].astype(f32))
    assert np.array_equal(g["constants"].view(np.uint32), np.array(Ref32.constants(rad.shape[1], rad.shape[0], float(g["delta_time"])), f32).view(np.uint32))
    for ops in ref.OPERATOR_SETS:
        counts, lum, ldr = ref.step(Ref32, rad, float(g["initial_luminance"]), float(g["delta_time"]), ops)
        assert np.array_equal(counts, g["counts"]) and f32(lum).view(np.uint32) == g["luminance"].view(np.uint32)
        assert ref.same_bits_or_class(ldr, g[f"ldr_{ops}"]).all()
