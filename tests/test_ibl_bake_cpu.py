"""The IBL bakes without a GPU: the C oracle (oracle/sailor_oracle.c, the kernels' bit-level twin) against the float64 restatements of oracle/oracle_f64.py on
every named case of tests/ibl_bake_cases.py, closed forms that need neither, the 2:1 chain bit for bit, and MUTANTS of the float64 laws: each wrong law
must break, on a named case, the allowance that tests/test_ibl_bake_gpu.py gives the kernels -- max(2 x the C oracle's error, the kernel's summation-tree
floor) -- by a factor of two, so that a kernel which followed the wrong law to within that allowance would still fail against the right one.

The C oracle's own error is printed per case and level and held to the bound of a sequential float sum: N roundings for the N terms of the numerator and,
in the pre-filter, N more for the weight."""
import numpy as np
import pytest

import ibl_bake_cases as bc
from fuzz_cases import nonfinite_mismatch
from oracle import oracle, oracle_f64 as f64

f32 = np.float32
PREFILTER_C_BOUND = 2 * 1024 * bc.U
IRRADIANCE_C_BOUND = 65536 * bc.U


def _id(case):
    return "-".join(str(v) for v in case)


# ---- the 2:1 chain ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,levels", bc.SIZES)
def test_mip_restatement_is_the_c_oracle_bit_for_bit(size, levels):
    """oracle_f64.generate_mipmaps_cube, written from include/sailor_hip.h, against the C oracle: odd sizes drop the last row and column, a 1 x 1 level
    repeats, 3e38 overflows to +inf the same way"""
    for name in ("alpha_noise", "sun_corner", "huge"):
        level0 = bc.cube(name, size, levels)[:6 * size * size * 4]
        mine, c = f64.generate_mipmaps_cube(level0, size, levels), oracle.generate_mipmaps_cube(level0, size, levels)
        assert mine.dtype == f32 and mine.size == oracle.cube_level_offsets(size, levels)[1]
        np.testing.assert_array_equal(mine.view(np.uint32), c.view(np.uint32))
    # the header's rule, spelled out on numbers: level 1 of a 3 x 3 face is the mean of its top-left 2 x 2 block
    if size == 3:
        l0 = np.arange(6 * 9 * 4, dtype=f32).reshape(6, 3, 3, 4)
        got = f64.generate_mipmaps_cube(l0, 3, 2)[6 * 9 * 4:].reshape(6, 1, 1, 4)
        np.testing.assert_array_equal(got[:, 0, 0], ((l0[:, 0, 0] + l0[:, 0, 1]) + (l0[:, 1, 0] + l0[:, 1, 1])) * f32(0.25))


# ---- the C oracle against float64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.PREFILTER_CASES, ids=_id)
def test_prefilter_c_oracle_against_float64(case):
    name, size, levels = case
    for level, roughness in bc.ladder(levels).items():
        ref, spread = bc.prefilter_f64(name, size, levels, level, roughness)
        c = bc.prefilter_c(name, size, levels, level, roughness)
        err = bc.bake_error(c, ref, bc.prefilter_scale(name, size, levels, level, roughness), spread)
        print(f"[prefilter f64] {name} {size}/{levels} level {level} roughness {roughness:.4f}: C oracle {err:.3e}")
        assert np.isfinite(c).all(), level
        assert bc.within_c_bound(c, ref, bc.prefilter_scale(name, size, levels, level, roughness), spread, PREFILTER_C_BOUND, size, bc.cube(*case)), (level, err)
        np.testing.assert_array_equal(c[..., 3], 1.0)


@pytest.mark.parametrize("case", bc.HOSTILE_ROUGHNESS_CASES, ids=_id)
def test_prefilter_c_oracle_at_hostile_roughness(case):
    name, size, levels, baked = case
    for level in baked:
        for roughness in bc.HOSTILE_ROUGHNESS:
            c = bc.prefilter_c(name, size, levels, level, roughness)
            if bc.alpha_is_zero(roughness):
                err, at_lod0 = bc.roughness_zero_error(c, name, size, levels, level)
                print(f"[prefilter f64] {name} {size}/{levels} level {level} roughness {roughness:g}: C oracle {err:.3e}, {at_lod0} of {c[..., 0].size} texels at lod 0")
                assert err <= PREFILTER_C_BOUND, (level, roughness, err)
            else:
                ref, spread = bc.prefilter_f64(name, size, levels, level, roughness)
                scale = bc.prefilter_scale(name, size, levels, level, roughness)
                print(f"[prefilter f64] {name} {size}/{levels} level {level} roughness {roughness:g}: C oracle {bc.bake_error(c, ref, scale, spread):.3e}")
                assert bc.within_c_bound(c, ref, scale, spread, PREFILTER_C_BOUND, size, bc.cube(name, size, levels)), (level, roughness)
            assert np.isfinite(c).all()
        nan = bc.prefilter_c(name, size, levels, level, float("nan"))   # no sample passes cosLi > 0: 0 / 0, as the shader
        assert np.isnan(nan[..., :3]).all() and (nan[..., 3] == 1.0).all()


@pytest.mark.parametrize("case", bc.IRRADIANCE_F64, ids=_id)
def test_irradiance_c_oracle_against_float64(case):
    ref, spread = bc.irradiance_f64(*case)
    c = bc.irradiance_c(*case)
    err = bc.bake_error(c, ref, bc.irradiance_scale(*case), spread)
    print(f"[irradiance f64] {_id(case)}: C oracle {err:.3e}")
    assert np.isfinite(c).all() and bc.within_c_bound(c, ref, bc.irradiance_scale(*case), spread, IRRADIANCE_C_BOUND, case[1], bc.cube(*case[:3])), err
    np.testing.assert_array_equal(c[..., 3], 1.0)


@pytest.mark.parametrize("case", bc.EQUIRECT_CASES, ids=_id)
def test_equirect_c_oracle_against_float64(case):
    """the bound: atan2f, the division, the scaling and the - 0.5 lose a few roundings of the tap coordinate, whose size is the image's: 8 U x the larger
    extent in texels, against an image whose steepest step is its whole range (the checker channel), plus the lerps"""
    kind, w, h, n, repeat = case
    err = bc.equirect_error(bc.equirect_c(*case), bc.equirect_f64(*case), bc.panorama(kind, w, h))
    print(f"[equirect f64] {_id(case)}: C oracle {err:.3e}")
    assert err <= 8 * bc.U * max(w, h) + bc.EQUIRECT_FLOOR, err


@pytest.mark.parametrize("case", bc.EQUIRECT_COVER_CASES, ids=_id)
def test_equirect_cover(case):
    kind, w, h, n = case
    img = bc.panorama(kind, w, h)
    whole = bc.equirect_f64(kind, w, h, n, True)
    for cover in bc.covers(w, h, n):
        canary = np.full((6, n, n, 4), -7.0)
        ref = f64.equirect_to_cube(img, n, cover=cover, out=canary.copy())
        c = oracle.equirect_to_cube(img, n, cover=cover, out=canary.astype(f32))
        cw, ch = min(cover[0], n), min(cover[1], n)
        inside = np.zeros((6, n, n), bool)
        inside[:, :ch, :cw] = True
        assert (c[~inside] == -7.0).all() and (ref[~inside] == -7.0).all()
        np.testing.assert_array_equal(ref[inside], whole[inside])
        assert inside.any() == (cw > 0 and ch > 0)
        if inside.any():
            assert bc.equirect_error(c[inside], ref[inside], img) <= 8 * bc.U * max(w, h) + bc.EQUIRECT_FLOOR


# ---- non-finite texels, by class --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.PREFILTER_NONFINITE, ids=_id)
def test_prefilter_nonfinite_by_class(case):
    name, size, levels = case
    seen = 0
    for level, roughness in bc.ladder(levels).items():
        c = bc.prefilter_c(name, size, levels, level, roughness)
        if name == "huge":   # 3e38 x the sum of cosLi overflows a float in every texel; float64 has no such sum to compare with
            assert np.isposinf(c[..., :3]).all()
        else:
            ref = bc.prefilter_f64(name, size, levels, level, roughness)[0]
            assert nonfinite_mismatch(c, ref) is None, (level, nonfinite_mismatch(c, ref))
            seen += int((~np.isfinite(c)).sum())
            fin = np.isfinite(ref)
            assert (np.abs(c[fin] - ref[fin]) <= PREFILTER_C_BOUND * np.abs(ref[fin]) + bc.prefilter_f64(name, size, levels, level, roughness)[1][fin]).all()
        np.testing.assert_array_equal(c[..., 3], 1.0)
    assert name == "huge" or seen > 0, "the hostile texel reached no output texel"


@pytest.mark.parametrize("case", bc.IRRADIANCE_NONFINITE, ids=_id)
def test_irradiance_nonfinite_by_class(case):
    c = bc.irradiance_c(*case)
    if case[0] == "huge":   # 2 x 3e38 is +inf before it is weighed; sample 0 has cosTheta = max(0, a rounding residue): inf x 0 = NaN in the texels where that is 0
        assert (np.isposinf(c[..., :3]) | np.isnan(c[..., :3])).all()
    else:
        ref = bc.irradiance_f64(*case)[0]
        assert nonfinite_mismatch(c, ref) is None, nonfinite_mismatch(c, ref)
        assert (~np.isfinite(c)).sum() > 0
    np.testing.assert_array_equal(c[..., 3], 1.0)


# ---- closed forms -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_constant_sky_stays_the_constant():
    """every output texel of every bake is the constant: to the pre-filter's sequential-sum bound, and to the quadrature error of the 65 536-point
    hemisphere set (2 mean(cos theta) = 1 - 1 / 65 536) plus the sum's bound for the irradiance"""
    want = np.float64(bc.CONSTANT[:3])
    for size, levels in bc.SIZES:
        for level, roughness in bc.ladder(levels).items():
            outs = [bc.prefilter_c("constant", size, levels, level, roughness)]
            if ("constant", size, levels) in bc.PREFILTER_CASES:
                outs.append(bc.prefilter_f64("constant", size, levels, level, roughness)[0])
            for out in outs:
                assert np.abs(out[..., :3] / want - 1.0).max() <= PREFILTER_C_BOUND
    for out in (bc.irradiance_c("constant", 8, 4, 1), bc.irradiance_f64("constant", 8, 4, 1)[0]):
        assert np.abs(out[..., :3] / want - 1.0).max() <= IRRADIANCE_C_BOUND + 2.0 / 65536
    eq = np.broadcast_to(bc.CONSTANT, (3, 7, 4))
    for repeat in (True, False):
        for out in (oracle.equirect_to_cube(eq, 5, repeat=repeat), f64.equirect_to_cube(eq, 5, repeat=repeat)):
            assert np.abs(out / np.float64(bc.CONSTANT) - 1.0).max() <= bc.EQUIRECT_FLOOR


@pytest.mark.parametrize("size,levels,roughness,want", [
    (16, 2, 1.0, 2.0),    # lod 0.5 log2(6 * 256 / 1024) + 1 = 1.29 for every sample: clamped to the last level
    (32, 3, 1.0, 3.0),    # 2.29 -> level 2
    (5, 3, 1.0, 1.0),     # 0.5 log2(6 * 25 / 1024) + 1 < 0: clamped to level 0
    (8, 4, 1.0, 2.0 + 0.5 * np.log2(6.0 * 64.0 / 1024.0)),   # not clamped: at roughness 1 the pdf is 1 / (4 PI) for every sample and PI cancels against wt
    (32, 6, 1.0, 2.0 + 0.5 * np.log2(6.0 * 1024.0 / 1024.0)),
])
def test_level_tagged_reads_the_lod_law_back(size, levels, roughness, want):
    """level l holds l + 1, so a texel is sum(cosLi (1 + lod_i)) / sum(cosLi); at roughness 1 the GGX pdf is constant, lod = 0.5 log2(6 size^2 / 1 024) + 1
    for every sample -- without either restatement"""
    level = levels - 1
    c = bc.prefilter_c("level_tagged", size, levels, level, roughness)
    r = f64.prefilter_env_level(bc.cube("level_tagged", size, levels), size, levels, level, roughness)
    assert np.abs(c[..., :3] - want).max() <= 1e-5 * want and np.abs(r[..., :3] - want).max() <= 1e-9 * want


def test_tagged_panorama_shows_the_taps():
    """r = column, g = row: where the float64 tap coordinates are at least 1e-3 from an integer (the floor cannot differ) and both taps are inside the image
    (no wrap: the tag is linear there), the C oracle's r and g ARE the tap coordinates, to the coordinate's own rounding"""
    w, h, n = 100, 37, 33
    px, py = f64.equirect_taps(w, h, n)
    c = bc.equirect_c("tagged", w, h, n, True)
    seen = 0
    for coord, extent, channel in ((px, w, 0), (py, h, 1)):
        ok = (np.abs(coord - np.round(coord)) >= 1e-3) & (coord >= 0.0) & (coord <= extent - 1.0)
        lo, frac = np.floor(coord[ok]), coord[ok] - np.floor(coord[ok])
        want = lo * (1.0 - frac) + (lo + 1.0) * frac
        assert np.abs(c[..., channel][ok] - want).max() <= 16 * bc.U * extent
        assert ((c[..., channel][ok] > lo - 1e-4) & (c[..., channel][ok] < lo + 1.0 + 1e-4)).all()
        seen += int(ok.sum())
    assert seen > 6 * n * n


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "lod law without the + 1": dict(lod_bias=0.0),
    "faces 2 and 3 swapped": dict(swap_faces_2_3=True),
    "texel centre for its corner": dict(texel_offset=0.5),
    "exact pi in the equirect pass": dict(equirect_pi=float(np.pi)),
    "cosLi weight dropped": dict(cos_weight=False),
}
APPLIES = {   # which entries read the law at all
    "lod law without the + 1": ("prefilter",), "faces 2 and 3 swapped": ("prefilter", "irradiance", "equirect"),
    "texel centre for its corner": ("prefilter", "irradiance", "equirect"),
    "exact pi in the equirect pass": ("equirect",), "cosLi weight dropped": ("prefilter",),
}
MUTANT_CASES = dict(   # small on purpose: a mutant costs a float64 bake per case
    prefilter=[("level_tagged", 8, 4), ("six_colours", 5, 3), ("sun_centre", 8, 4), ("smooth", 5, 3)],
    irradiance=[("six_colours", 8, 4, 2), ("sun_centre", 8, 4, 2)],
    equirect=[("tagged", 256, 128, 1, True), ("tagged", 256, 128, 2, True), ("tagged", 7, 3, 5, False), ("sun", 100, 37, 8, True)],
)


def _mutant_margins(entry, law):
    """per named case (and level): the mutant's error against the true float64 reference over the kernels' allowance there"""
    law = dict(f64.BAKE_LAW, **law)
    out = {}
    for case in MUTANT_CASES[entry]:
        if entry == "prefilter":
            name, size, levels = case
            for level, roughness in bc.ladder(levels).items():
                ref, spread = bc.prefilter_f64(name, size, levels, level, roughness)
                scale = bc.prefilter_scale(name, size, levels, level, roughness)
                allow = bc.allowance(bc.bake_error(bc.prefilter_c(name, size, levels, level, roughness), ref, scale, spread), bc.PREFILTER_FLOOR)
                mutant = f64.prefilter_env_level(bc.cube(name, size, levels), size, levels, level, roughness, law=law)
                out[case + (level,)] = bc.bake_error(mutant, ref, scale, spread) / allow
        elif entry == "irradiance":
            ref, spread = bc.irradiance_f64(*case)
            scale = bc.irradiance_scale(*case)
            allow = bc.allowance(bc.bake_error(bc.irradiance_c(*case), ref, scale, spread), bc.IRRADIANCE_FLOOR)
            mutant = f64.compute_irradiance_map(bc.cube(*case[:3]), case[1], case[2], case[3], law=law)
            out[case] = bc.bake_error(mutant, ref, scale, spread) / allow
        else:
            kind, w, h, n, repeat = case
            img, ref = bc.panorama(kind, w, h), bc.equirect_f64(*case)
            allow = bc.allowance(bc.equirect_error(bc.equirect_c(*case), ref, img), bc.EQUIRECT_FLOOR)
            out[case] = bc.equirect_error(f64.equirect_to_cube(img, n, repeat=repeat, law=law), ref, img) / allow
    return out


def test_swapping_the_hammersley_coordinates_is_no_mutant():
    """(i / N, RadicalInverse_VdC(i)) for i < N = 2^k: N x the radical inverse is the k-bit reversal of i, an involution, so the swapped pairs are the SAME
    set of points in another order, and both coordinates are exact in float.  No case can tell the two laws apart (beyond the order of a sum), and none
    has to: the law is pinned by this identity instead."""
    for n in (1024, 65536):
        u1, u2 = f64._hammersley(n)
        s1, s2 = f64._hammersley(n, dict(f64.BAKE_LAW, swap_hammersley=True))
        assert sorted(zip(u1, u2)) == sorted(zip(s1, s2))
        assert (np.float64(f32(u1)) == u1).all() and (np.float64(f32(u2)) == u2).all()
    case = ("sun_centre", 8, 4)
    ref = bc.prefilter_f64(*case, 1, bc.ladder(4)[1])[0]
    swapped = f64.prefilter_env_level(bc.cube(*case), 8, 4, 1, bc.ladder(4)[1], law=dict(f64.BAKE_LAW, swap_hammersley=True))
    assert np.abs(swapped / ref - 1.0).max() < 1e-12


@pytest.mark.parametrize("mutant,entry", [(m, e) for m in MUTANTS for e in APPLIES[m]], ids=lambda v: v.replace(" ", "_"))
def test_a_wrong_law_breaks_the_allowance_on_a_named_case(mutant, entry):
    margins = _mutant_margins(entry, MUTANTS[mutant])
    best = max(margins, key=margins.get)
    print(f"[mutant] {mutant} / {entry}: caught by {_id(best)} at {margins[best]:.3g} x the allowance; " +
          ", ".join(f"{_id(k)} {v:.3g}" for k, v in margins.items()))
    assert margins[best] > 2.0, margins
