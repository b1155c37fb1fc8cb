"""CPU suite of the star points and the sun-shaft pass: ABI, the host functions (temperature table, star mesh, model matrix) against the fp32 restatement of
tests/stars_ref.py bit for bit, every (spectral, sub-type) byte pair, truncated catalogues, the fp32 restatement held against its float64 twin on every
case, the coverage the cases must have, and the golden file.  No GPU needed."""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import stars_cases as sc
import stars_ref as sref
from sailor_amd import _lib, host

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
R32, R64 = sref.Ref32(), sref.Ref64()
SYMBOLS = ("sailor_hip_sky_sun_shafts", "sailor_hip_sky_stars", "sailor_hip_sky_stars_workspace_bytes", "sailor_hip_sky_stars_bind_workspace",
           "sailor_host_sky_star_color_table", "sailor_host_sky_star_mesh", "sailor_host_sky_stars_model")
CAP = 0.02   # the share of a case's texels or stars that may take another branch or tap in the twin and be left out of the value comparison
INVALID = -1
FP = C.POINTER(C.c_float)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def fp(a):
    return a.ctypes.data_as(FP)


def test_abi_symbols_and_documentation():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    declared = set(re.findall(r"\b(sailor_(?:hip|host)_\w+)\s*\(", header))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.sailor_hip_version() >= 8
    design = (ROOT / "DESIGN.md").read_text()
    assert "Not drawn" not in header and "*Not drawn*" not in design
    assert "sky_stars.hip" in (ROOT / "sailor_amd" / "csrc" / "Makefile").read_text()
    assert lib.sailor_hip_sky_stars_workspace_bytes(0) == 0 and lib.sailor_hip_sky_stars_workspace_bytes(-1) == 0
    assert lib.sailor_hip_sky_stars_workspace_bytes(65537) == 0 and lib.sailor_hip_sky_stars_workspace_bytes(65536) == 65536 * 20
    assert lib.sailor_hip_sky_stars_workspace_bytes(9110) == 9110 * 16 + 36448   # the pixel ids rounded up to 16 bytes


# ---- the host functions ---------------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_the_catalogue_and_the_colour_rows():
    data, rows = sc.catalogue(), sc.color_rows()
    assert len(data) == 28 + 32 * 9110 and struct.unpack_from("<7i", data) == (0, 1, -9110, 1, 1, 1, 32)   # a negative count: J2000 (abs() at SkyNode.cpp:66)
    assert rows.shape == (782, 11) and rows.dtype == f32 and rows[0, 0] == 1000 and rows[-1, 0] == 40000
    _, _, spectral, sub, mag = R32.parse(data)
    assert {ord(" "), ord("p")} <= set(spectral.tolist()), "the spectral bytes outside 'A' .. 'Y'"
    assert {ord(x) for x in "mpeNIC+/ "} <= set(sub.tolist()), "the sub-type bytes that are no digit"
    assert int((mag.astype(np.int64) + 40 < 0).sum()) == 2, "Sirius and Canopus: a negative divisor"


def test_color_table_against_ref32():
    rows = sc.color_rows()
    got, want = host.sky_star_color_table(rows), R32.color_table(rows)
    assert got.shape == (391, 3) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(got[0], rows[1, 5:8]) and np.array_equal(got[390], rows[-1, 5:8]), "the later of two rows of a temperature wins; index 390 is addressed"
    assert not (got == 0).all(1).any()
    # rows outside the table's range land on its ends, a NaN temperature on row 0
    odd = np.zeros((4, 11), f32)
    odd[:, 0] = (-5.0e9, 1.0e30, np.nan, 39949.0)
    odd[:, 5] = (1.0, 2.0, 3.0, 4.0)
    got, want = host.sky_star_color_table(odd), R32.color_table(odd)
    assert np.array_equal(bits(got), bits(want)) and got[0, 0] == 3.0 and got[390, 0] == 2.0 and got[389, 0] == 4.0 and np.count_nonzero(got) == 3
    lib = _lib.load()
    assert lib.sailor_host_sky_star_color_table(None, 1, fp(got)) == INVALID and lib.sailor_host_sky_star_color_table(fp(odd), 4, None) == INVALID


def test_star_mesh_of_the_fixture_against_ref32():
    table = host.sky_star_color_table(sc.color_rows())
    pos, col = host.sky_star_mesh(sc.catalogue(), table)
    want_pos, want_col, divisor = sc.fixture_mesh()
    assert pos.shape == (9110, 3) and col.shape == (9110, 4)
    assert np.array_equal(bits(pos), bits(want_pos)) and np.array_equal(bits(col), bits(want_col))
    assert np.isfinite(pos).all() and (col[:, 3] == 1).all() and col[:, :3].min() >= 0 and col[:, :3].max() <= 1
    mirrored = np.flatnonzero(divisor < 0)
    assert len(mirrored) == 2, "a negative divisor mirrors the star, as written"
    ra, dec = (a.astype(f32) for a in R32.parse(sc.catalogue())[:2])
    for s in mirrored:   # the star lies opposite to its direction on the sky
        direction = np.array([np.sin(ra[s]) * np.cos(dec[s]), np.cos(ra[s]) * np.cos(dec[s]), np.sin(dec[s])])
        assert np.dot(direction, pos[s]) < 0
    radius = np.linalg.norm(pos.astype(np.float64), axis=1)
    assert 590 < radius.min() and radius.max() < 16000   # 5000 / (7.96 + 0.4) .. 5000 / |-0.72 + 0.4|, inside the synthetic camera's zFar
    p64, c64, _ = R64.star_mesh(sc.catalogue(), R64.color_table(sc.color_rows()))
    assert np.abs(pos - p64).max() <= 2e-6 * np.abs(p64).max() and np.abs(col - c64).max() <= 1e-6


def sweep_catalogue():
    """65 536 entries, one per (spectral, sub-type) byte pair"""
    n = 65536
    e = np.zeros((n, 32), np.uint8)
    e[:, 20], e[:, 21] = np.arange(n) >> 8, np.arange(n) & 255
    e[:, 22:24] = np.full(n, 300, "<i2").view(np.uint8).reshape(n, 2)
    return struct.pack("<7i", 0, 1, -n, 1, 1, 1, 32) + e.tobytes()


def test_every_spectral_and_sub_type_byte_pair_against_ref32():
    table = host.sky_star_color_table(sc.color_rows())
    pos, col = host.sky_star_mesh(sweep_catalogue(), table)
    want, rows = R32.byte_pair_colors(R32.color_table(sc.color_rows()))
    assert np.array_equal(bits(col), bits(want.reshape(-1, 4)))
    assert rows.min() == 0 and rows.max() == 390 and len(np.unique(rows)) > 300, "both ends of the table are reached"
    assert np.array_equal(bits(pos), np.tile(bits(pos[:1]), (65536, 1)))
    # a table of row numbers shows the row each pair addresses, whatever the colours are
    marker = np.repeat(np.arange(391, dtype=f32), 3)
    _, col = host.sky_star_mesh(sweep_catalogue(), marker)
    got_rows = np.rint(col[:, 0].astype(np.float64) ** 2.2).astype(np.int64).reshape(256, 256)
    assert np.array_equal(got_rows, rows)
    a9 = R32.temperature_row(R32.temperature(np.uint8(ord("A")), np.uint8(ord("9"))))
    a0 = R32.temperature_row(R32.temperature(np.uint8(ord("A")), np.uint8(ord("0"))))
    assert (a9, a0) == (63, 90), "A9 is 7300 K, A0 7300 + 9 * 300 K"
    assert rows[ord(" "), ord("5")] == 0 and rows[ord("p"), ord(" ")] == 0, "an unknown spectral byte takes the range {0, 0}"
    assert rows[ord("O"), ord("+")] == 390, "'9' - '+' = 14 steps of 1111 K above 30000 K: beyond the table"
    assert rows[ord("O"), ord("e")] == 390, "'9' - 'e' = -44 wraps to 2^32 - 44, times 1111 to 2^32 - 48884: a temperature of 4.29e9 K"
    assert rows[ord("Y"), ord("9")] == 0 and rows[ord("D"), ord("9")] == 390, "0 K: 0 / 100 - 10 wraps and is negative as an int32; 100 000 K"


def test_truncated_and_short_catalogues_are_refused():
    lib = _lib.load()
    data, table = sc.catalogue(), host.sky_star_color_table(sc.color_rows()).reshape(-1)
    pos, col, count = np.full((9111, 3), 7.0, f32), np.full((9111, 4), 7.0, f32), C.c_uint32(123)

    def mesh(b, n=None, cap=9111, t=table, p=pos, c=col, k=count):
        return lib.sailor_host_sky_star_mesh(b, len(b) if n is None else n, None if t is None else fp(t), None if p is None else fp(p), None if c is None else fp(c),
                                             cap, None if k is None else C.byref(k))

    for cut in (0, 1, 27, 28, 29, 28 + 31, 28 + 32 * 9110 - 1, 28 + 32 * 9109):
        assert mesh(data[:cut]) == INVALID, cut
        with pytest.raises(ValueError):
            R32.parse(data[:cut])
    assert mesh(data, n=len(data) - 1) == INVALID
    assert (pos == 7.0).all() and (col == 7.0).all() and count.value == 123, "a refused catalogue writes nothing"
    huge = bytearray(data)
    for value in (-2 ** 31, 2 ** 31 - 1, 9111, -9111):
        struct.pack_into("<i", huge, 8, value)
        assert mesh(bytes(huge)) == INVALID, value
    assert mesh(data, cap=9109) == INVALID and count.value == 9110 and (pos == 7.0).all(), "too little room: the count is reported, nothing is written"
    assert lib.sailor_host_sky_star_mesh(None, 100, fp(table), fp(pos), fp(col), 9111, C.byref(count)) == INVALID
    assert mesh(data, t=None) == INVALID and mesh(data, p=None) == INVALID and mesh(data, c=None) == INVALID and mesh(data, k=None) == INVALID
    empty = struct.pack("<7i", 0, 1, 0, 1, 1, 1, 32)
    assert mesh(empty) == 0 and count.value == 0
    assert mesh(data) == 0 and count.value == 9110 and (pos[9110] == 7.0).all()
    with pytest.raises(_lib.SailorHipError):
        host.sky_star_mesh(data[:-1], table)


@pytest.mark.parametrize("camera", [(0.0, 0.0, 0.0), (10.0, 150.0, -20.0), (-3.0e5, 1.5e6, 2.5e5)])
def test_model_matrix_against_ref32_and_a_float64_quaternion_product(camera):
    got = host.sky_stars_model(camera)
    assert np.array_equal(bits(got), bits(R32.stars_model(camera)))
    # float64, by the textbook: q = rz * rx * rz as Hamilton products, the rotation matrix of a unit quaternion, the translation in the last column
    def q(angle, axis):
        return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * np.asarray(axis, np.float64)])

    def hamilton(a, b):
        return np.concatenate([[a[0] * b[0] - a[1:] @ b[1:]], a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:])])

    rz, rx = q(float(f32(0.01118)), (0, 0, 1)), q(float(f32(-0.00972)), (1, 0, 0))
    w, x, y, z = hamilton(hamilton(rz, rx), rz)
    rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                    [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = rot, np.asarray(camera, f32).astype(np.float64)
    m = got.astype(np.float64).reshape(4, 4).T
    assert np.abs(m[:3, :3] - rot).max() <= 2.0 ** -22, "a few fp32 roundings of values of at most 1"
    assert np.array_equal(m[:, 3], want[:, 3]) and np.array_equal(m[3], want[3])
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-15 and np.abs(m[:3, :3] @ m[:3, :3].T - np.eye(3)).max() < 1e-6
    assert np.abs(np.asarray(R64.stars_model(camera)).reshape(4, 4).T - want).max() < 1e-15
    lib = _lib.load()
    assert lib.sailor_host_sky_stars_model(None, fp(got)) == INVALID and lib.sailor_host_sky_stars_model(fp(got), None) == INVALID


# ---- Ref32 against Ref64 ------------------------------------------------------------------------------------------------------------------------------
# measured on the cases of stars_cases.py (this file prints them; DESIGN.md section 4 carries them):
#   shafts: texels with a differing tap, max |d| / plane max over the finite words of the other texels
MEASURED_SHAFTS = {
    "in_view_60":  (0, 5.64e-07),
    "in_view_100": (0, 4.90e-07),
    "in_view_1":   (0, 1.51e-06),
    "fading_7":    (0, 8.42e-07),
    "behind_60":   (0, 1.22e-08),
    "dark_100":    (0, 1.45e-08),
}
#   stars: stars that take another branch, pixel or tap, max |d fragment rgb| / largest fragment rgb, max |d target| / target max with those stars left out
MEASURED_STARS = {
    "fixture_96":    (0, 5.86e-05, 1.03e-06),
    "fixture_131":   (0, 3.49e-05, 1.70e-06),
    "synthetic_96":  (1, 1.84e-03, 1.70e-05),
    "synthetic_131": (0, 6.24e-03, 9.30e-05),
}
# The stars' deviation is the mask's: 1 - 1000 * length(viewportPos - fragUV) multiplies the fp32 error of a star's NDC position (a few 1e-7 after the matrix
# product and the division by w) by a thousand.  The bound is 4 x the measured figure of the case itself, per quantity.


def shaft_twin(name):
    c = sc.shaft_case(name)
    a, ia, U = sc.shaft_reference(name)
    b, ib, U64 = sc.run_shafts(R64, c)
    assert U["early"] == U64["early"]
    differ = np.zeros(a.shape[:2], bool) if ia["taps"] is None else (ia["taps"] != ib["taps"]).any(axis=(0, 3))
    use = np.isfinite(a) & ~differ[..., None]
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    with np.errstate(invalid="ignore"):   # the hostile texel: inf - inf
        return int(differ.sum()), float(differ.mean()), float(np.abs(a - b)[use].max() / np.abs(a[use]).max())


@pytest.mark.parametrize("name", [c.name for c in sc.SHAFT_CASES])
def test_shafts_fp32_restatement_against_the_float64_twin(name):
    n, share, d = shaft_twin(name)
    print(f"{name}: a tap differs on {n} texels ({share:.4f}), max |d| / plane max {d:.3g}")
    measured = MEASURED_SHAFTS[name]
    assert share <= CAP and n <= 4 * measured[0] and d <= 4.0 * measured[1], (name, n, d)


def star_twin(name):
    c = sc.star_case(name)
    a, S = sc.star_reference(name)
    _, T = sc.run_stars(R64, c)
    drawn = S["drop"] == 0
    differ = (S["drop"] != T["drop"]) | (drawn & ((S["px"] != T["px"]) | (S["py"] != T["py"]) | (S["sky"] != T["sky"]) | (S["taps"] != T["taps"]).any(-1)))
    use = drawn & ~differ
    assert np.array_equal(S["frag"][use][:, 3], T["frag"][use][:, 3])   # alpha is 1, or 0 on an Earth hit
    d_frag = float(np.abs(S["frag"] - T["frag"])[use][:, :3].max() / np.abs(S["frag"][use][:, :3]).max())
    target = sc.star_inputs(name)[5]
    x, y = R32.stars_blend(S, target, c.w, c.h, skip=differ), R64.stars_blend(T, target, c.w, c.h, skip=differ)
    return int(differ.sum()), float(differ.mean()), d_frag, float(np.abs(x - y).max() / np.abs(x).max())


@pytest.mark.parametrize("name", [c.name for c in sc.STAR_CASES if c.stars != "empty"])
def test_stars_fp32_restatement_against_the_float64_twin(name):
    n, share, d_frag, d_target = star_twin(name)
    print(f"{name}: {n} stars differ in a branch, pixel or tap ({share:.4f}), max |d fragment| / largest fragment {d_frag:.3g}, max |d target| / target max {d_target:.3g}")
    measured = MEASURED_STARS[name]
    assert share <= CAP and n <= 4 * measured[0] and d_frag <= 4.0 * measured[1] and d_target <= 4.0 * measured[2], (name, n, d_frag, d_target)


def test_design_document_carries_the_measured_twin_figures():
    """DESIGN.md section 4 states the figures this file asserts four times of, in this format"""
    text = (ROOT / "DESIGN.md").read_text()
    for name, (n, d) in MEASURED_SHAFTS.items():
        assert f"`{name}` {n} / {d:.2e}" in text, name
    for name, (n, f, t) in MEASURED_STARS.items():
        assert f"`{name}` {n} / {f:.2e} / {t:.2e}" in text, name


# ---- coverage, asserted from Ref32 so that the cases are known to reach it ---------------------------------------------------------------------------
def test_shaft_cases_reach_every_edge_both_early_outs_and_the_sun_behind_the_camera():
    assert {c.distance for c in sc.SHAFT_CASES} == {1, 7, 60, 100}
    assert {(c.w, c.h) for c in sc.SHAFT_CASES} == {(96, 64), (131, 77)} and {c.cw for c in sc.SHAFT_CASES} == {32, 38}
    for c in sc.SHAFT_CASES:
        out, info, U = sc.shaft_reference(c.name)
        target = sc.shaft_target(c)
        if c.kind == "in_view":
            assert not U["early"] and 0 < U["uvx"] < 1 and 0 < U["uvy"] < 1 and U["mixTerm"] == 1
            assert all(e > 0 for e in info["edges"]), (c.name, info["edges"])   # taps clamped at the left, right, top and bottom edge
            assert (bits(out) != bits(target)).mean() > 0.5
        elif c.kind == "fading":
            assert not U["early"] and 1 < U["uvx"] < 1.51 and U["fade"] > 0 and 0 < U["mixTerm"] < 1
        elif c.kind == "behind":
            assert U["early"] and 0 < U["w"] < 0.1 and U["uvx"] > 1.51, "the sun behind the camera: a small w, uvView far outside"
        else:
            assert U["early"] and U["intensity"] == 0 and 0 < U["uvx"] < 1, "only the intensity returns early"
        if U["early"]:   # (0, 0, 0, 0) is still blended: rgb = 0 d + 0 (1 - Ad) + d (1 - 0), a = 0 - Ad Ad
            fin = np.isfinite(target).all(-1)
            assert np.array_equal(out[fin][:, :3], target[fin][:, :3]) and np.array_equal(out[fin][:, 3], -(target[fin][:, 3] ** 2))
            assert np.isnan(out[~fin][:, :3]).all(), "0 * inf"
    # a NaN uvView fails every comparison and falls through to the loop
    c = sc.shaft_case("in_view_60")
    frame = sc.shaft_frame(c)
    frame.projection[15] = float("nan")
    U = R32.shaft_uniforms(frame, sc.shaft_params(c), c.cw, c.cw)
    assert np.isnan(U["uvx"]) and not U["early"]


def test_star_cases_reach_every_drop_collisions_edges_the_earth_and_the_mask():
    seen = 0
    for c in sc.STAR_CASES:
        if c.stars == "empty":
            continue
        out, S = sc.star_reference(c.name)
        drawn = S["drop"] == 0
        per_pixel = sc.stars_per_pixel(S, c.w)
        assert max(per_pixel.values()) >= 3, c.name
        assert (drawn & ~S["sky"]).sum() >= 3 and (drawn & S["sky"] & (S["mask"] > 0)).sum() >= 10 and (drawn & (S["mask"] < 1)).sum() >= 10, c.name
        target = sc.star_inputs(c.name)[5]
        ids = S["py"] * c.w + S["px"]
        lit_pixels = set(ids[drawn & S["sky"]].tolist())
        earth = [s for s in np.flatnonzero(drawn & ~S["sky"]) if ids[s] not in lit_pixels and (bits(target[S["py"][s], S["px"][s]]) == 0x80000000).all()]
        assert len(earth) >= 3 and all((bits(out[S["py"][s], S["px"][s]]) == 0).all() for s in earth), "-0 + 0 = +0 under the horizon"
        if c.stars == "synthetic":
            for bit in (sref.DROP_NONFINITE, sref.DROP_W, sref.DROP_X_LOW, sref.DROP_X_HIGH, sref.DROP_Y_LOW, sref.DROP_Y_HIGH, sref.DROP_Z_LOW, sref.DROP_Z_HIGH):
                assert ((S["drop"] & bit) != 0).sum() >= 1, (c.name, bit)
            assert (S["drop"][18:20] == sref.DROP_NONFINITE).all() and S["drop"][11] == sref.DROP_W
            a, b = sc.PIXEL_A[1] * c.w + sc.PIXEL_A[0], sc.PIXEL_B[1] * c.w + sc.PIXEL_B[0]
            assert per_pixel[a] == 4 and per_pixel[b] == 3 and per_pixel[sc.PIXEL_EARTH[1] * c.w + sc.PIXEL_EARTH[0]] == 3
            if c.w % 2 == 0 and c.h % 2 == 0:   # the star on the view axis: the corner of four pixels, goes right / down
                assert S["edge"][10] and drawn[10] and (S["px"][10], S["py"][10]) == (c.w // 2, c.h // 2)
                seen += 1
        else:
            assert ((S["drop"] & sref.DROP_W) != 0).sum() > 1000 and all(((S["drop"] & b) != 0).sum() > 100 for b in (4, 8, 16, 32))
    assert seen == 1
    assert int((sc.fixture_mesh()[2] < 0).sum()) == 2, "the mirrored stars of the fixture"


def test_star_order_matters_and_the_restatement_keeps_it():
    """the four stars of PIXEL_A summed in index order differ, in the last bits, from the same stars summed in another order: the order is observable"""
    c = sc.star_case("synthetic_96")
    out, S = sc.star_reference(c.name)
    target = sc.star_inputs(c.name)[5]
    px, py = sc.PIXEL_A
    on = np.flatnonzero((S["drop"] == 0) & (S["px"] == px) & (S["py"] == py))
    assert len(on) == 4
    forward = target[py, px].copy()
    for s in on:
        forward = forward + S["frag"][s]
    assert np.array_equal(bits(forward), bits(out[py, px])) and forward[3] == 4.0


# ---- the golden file --------------------------------------------------------------------------------------------------------------------------------
def test_golden_outputs():
    g = np.load(ROOT / "tests" / "golden" / "tiny_stars.npz")
    assert np.array_equal(bits(sc.shaft_reference(str(g["shafts_case"]))[0]), g["shafts_bits"])
    out, S = sc.star_reference(str(g["stars_case"]))
    assert np.array_equal(bits(out), g["stars_bits"]) and np.array_equal(S["drop"], g["drop"]) and np.array_equal(S["py"] * 96 + S["px"], g["pixels"])
    positions, colors, _ = sc.fixture_mesh()
    assert np.array_equal(bits(positions[:64]), g["first_positions_bits"]) and np.array_equal(bits(colors[:64]), g["first_colors_bits"])
    assert np.array_equal(bits(R32.color_table(sc.color_rows())), g["table_bits"])
    assert np.array_equal(bits(host.sky_stars_model((10.0, 150.0, -20.0))), g["model_bits"])
