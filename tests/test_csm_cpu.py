"""The directional shadow term (Standard.shader:266-283, Lighting.glsl:168-284) on the CPU: the fp32 C oracle against the float64 restatement on every
case of tests/csm_cases.py, what each case reaches counted on the reference's own decisions, a known answer for EVSM worked by hand, and the
`no map bound` rule.  tests/test_csm_gpu.py holds the kernels to the same references."""
import numpy as np
import pytest

import csm_cases
from oracle import oracle, oracle_f64

CASES = list(csm_cases.CASES)


@pytest.mark.parametrize("name", CASES)
def test_c_oracle_shadow_cases_agree_with_the_float64_restatement(name):
    """C oracle against oracle_f64.shade under the K2 bound 1e-4 |ref| + 1e-7 max |ref| on every pixel the reference does not leave out
    (want_shadow_margin: a discrete decision of the shadow term within 2 K 2^-24 A of flipping, or the first-order bound on the EVSM factor's fp32
    error beyond the pixel's tolerance); a pixel left out for undecided PCF taps alone stays within that many sixteenths of the unshadowed term;
    alpha bit for bit.  At most 1 % of a case's pixels are left out, and a pixel placed ON a cascade threshold or a rejection limit, or one float
    beside it, has its cascade and its rejection decided (the chain to it is exact in fp32: the tie is the strict compare's false side in both).

    Measured (CPU; pixels left out / of them for taps alone / pixels beyond the bound had none been left out / worst err / tol over the kept ones):
      ortho-ramp-synth 1 / 0 / 1 / 0.08           ortho2-ramp-synth-small 0 / 0 / 0 / 0.04     persp-ramp-penumbra_2_5 41 / 1 / 0 / 0.15
      persp-ramp-pcf_r32f-small 2 / 0 / 0 / 0.10  persp_one-mixed-penumbra_12 0 / 0 / 0 / 0.23 ortho-boundaries-pcf_r32f 3 / 2 / 1 / 0.36
      scaled-checker-pcf_rgba 2 / 2 / 0 / 0.05    ortho-checker-evsm_on_r16f 0 / 0 / 0 / 0.05  ortho-ramp-evsm_front 0 / 0 / 0 / 0.06
      ortho-ramp-evsm_behind 0 / 0 / 0 / 0.08     reject-evsm 0 / 0 / 0 / 0.05                 reject-pcf 0 / 0 / 0 / 0.03
      evsm_states 0 / 0 / 0 / 0.01                size-1x1 0 / 0 / 0 / 0.03                    size-2x2 1 / 0 / 0 / 0.05
      size-5x40 2 / 0 / 0 / 0.03                  size-64x3 2 / 0 / 0 / 0.03                   size-64x3-pcf 0 / 0 / 0 / 0.01
      missing-0 .. missing-all 0 / 0 / 0 / at most 0.05
    (6144 pixels in the 96 x 64 cases, 960 in the 40 x 24 ones.)"""
    case, ref, margin, c_ref = csm_cases.reference(name)
    out = margin["left_out"]
    worst = csm_cases.check_against_float64(c_ref, ref, margin, name)
    beyond = int((csm_cases.k2_excess(c_ref, ref) > 1.0).sum())
    print(f"[csm f64] {name}: C oracle worst err / tol {worst:.3f}, {out.sum()} of {out.size} pixels left out ({margin['taps_only'].sum()} for taps alone), "
          f"{beyond} beyond the bound with nothing left out")
    assert out.sum() <= 0.01 * out.size, f"{out.sum()} of {out.size} pixels left out"
    m0 = margin["lights"].get(0)
    if m0 is not None:
        assert m0["edges_decided"][case.boundary].all(), "a pixel on a threshold or a rejection limit is left out merely for being there"


@pytest.mark.parametrize("name", CASES)
def test_shadow_cases_reach_what_they_exist_for(name):
    """No case passes vacuously: the counts csm_cases.coverage() takes from the float64 reference's own decisions -- quadrants (a quadrant is a wave)
    whose 64 lanes are all / none / some behind the moment for each EVSM pair, quadrants that take the second early return (not all behind the
    positive moment, all behind the negative one), mixed-cascade and single-cascade quadrants, pixels per cascade, the histogram of PCF sixteenths,
    pixels rejected by each of the five compares, pixels with a partial EVSM factor -- are non-zero where the case names them.

    Measured: mixed-cascade quadrants 40 of 96 on the ramp, 48 of 96 on `mixed`, all 15 on `checker`; evsm_states 4 / 8 / 3 quadrants all / none / some
    behind the positive moment, 8 / 4 / 3 the negative, 4 take the second return; persp-ramp-penumbra_2_5 7 some (positive), 3 some (negative), 2422
    partial factors; persp_one-mixed-penumbra_12 7 / 5 / 4 and 1 / 11 / 4, 716 partial; reject-evsm and reject-pcf 96 / 120 / 96 / 80 / 264 pixels by
    compare; PCF sixteenths 1 .. 15 between 44 pixels (ortho2-ramp-synth-small) and 2124 (persp_one-mixed-penumbra_12)."""
    case, _ref, margin, _c = csm_cases.reference(name)
    cov = csm_cases.coverage(case, margin)
    print(f"[csm coverage] {name}: {cov}")
    for key in case.expect:
        assert cov[key] > 0, (key, cov)
    if name in csm_cases.MISSING:
        m0 = margin["lights"][0]
        absent = np.isin(m0["cascade"], csm_cases.MISSING[name])
        assert absent.any() and (m0["kind"][absent] == 0).all() and (m0["factor"][absent] == 1.0).all()
        assert (m0["kind"][~absent] != 0).all()


def test_the_cases_together_reach_every_branch():
    """What the header of the issue lists as never run: projective light matrices on both look-ups (w != 1 in every lane, and in some lanes only), a
    view matrix with w = 2, R32F and RGBA32F maps on the PCF cascades, an R16F map under EVSM, absent maps, windows narrower than a map and maps
    narrower than a window, and every wave state of both early returns."""
    built = {n: csm_cases.build(n) for n in CASES}
    fmt = lambda m: None if m is None else (m.dtype, m.ndim)
    kinds = {(k, fmt(m)) for c in built.values() for k, m in enumerate(c.frame.shadows.maps)}
    for want in [(1, (np.dtype(np.float32), 2)), (2, (np.dtype(np.float32), 3)), (0, (np.dtype(np.float16), 2)), (0, None), (3, None), (1, (np.dtype(np.float16), 2))]:
        assert want in kinds, want
    sizes = {m.shape[:2] for c in built.values() for m in c.frame.shadows.maps if m is not None}
    assert {(1, 1), (2, 2), (40, 5), (3, 64)} <= sizes
    view = lambda c: np.frombuffer(bytes(c.frame.cam.frame.view), np.float32)
    assert view(built["scaled-checker-pcf_rgba"])[15] == 2.0 and view(built["ortho-ramp-synth"])[15] == 1.0
    w_rows = lambda n: built[n].frame.shadows.lights_matrices.reshape(4, 4, 4)[:, :, 3]
    assert (w_rows("persp-ramp-penumbra_2_5")[:, :3] != 0).any(1).all()                       # all four cascades projective
    assert (w_rows("persp_one-mixed-penumbra_12")[:, :3] != 0).any(1).tolist() == [False, True, False, False]
    total = {}
    for n in CASES:
        case, _r, margin, _c = csm_cases.reference(n)
        for k, v in csm_cases.coverage(case, margin).items():
            if isinstance(v, int):
                total[k] = total.get(k, 0) + v
    for k in ("evsm_pos_all", "evsm_pos_none", "evsm_pos_some", "evsm_neg_all", "evsm_neg_none", "evsm_neg_some", "evsm_second_return", "evsm_partial",
              "mixed_quadrants", "uniform_quadrants", "pcf_partial", "reject_each"):
        assert total[k] > 0, k


def shadow_factor(shade, case):
    """radiance with the case's maps over radiance without any, per pixel and channel"""
    f = case.frame
    W, H = f.cam.width, f.cam.height
    g, idx, _ = oracle.light_cull(f.cam.frame, W, H, f.lights, f.depth)
    lit = shade(f, g, idx, True)[..., :3].astype(np.float64)
    unshadowed = shade(f, g, idx, False)[..., :3].astype(np.float64)
    assert (unshadowed > 0).all()
    return lit / unshadowed


def c_shade(f, g, idx, with_maps):
    csm = oracle.make_csm(f.shadows.lights_matrices, f.shadows.maps) if with_maps else (None, None)
    return oracle.shade(f.cam.frame, f.cam.width, f.cam.height, f.surface, f.lights, g, idx, csm[0])


def f64_shade(f, g, idx, with_maps):
    return oracle_f64.shade(bytes(f.cam.frame), f.cam.width, f.cam.height, f.surface, f.lights, g, idx, (f.shadows.lights_matrices, f.shadows.maps) if with_maps else None)


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_known_answer_evsm_two_level(p):
    """EVSM from its definition (Lighting.glsl:218-240, :263-284), using neither implementation.  The map holds the constant moments of the depth
    distribution p delta(z1) + (1 - p) delta(z2), z1 = 0.3 < z2 = 0.5 (reversed Z: z2 is the nearer occluder): for the warp Y = -exp(-40 z) the two
    values y1 < y2 with masses p, 1 - p, mean mu = p y1 + (1 - p) y2, variance p (1 - p) (y2 - y1)^2 -- e^-24 against a floor of 0; the positive warp's
    e^40 / 5 against its floor of 0.01.
    Chebyshev's bound variance / (variance + (t - mu)^2) at t = y2, where t - mu = p (y2 - y1), is p (1 - p) / (p (1 - p) + p^2) = 1 - p: attained, the
    mass at or above t.  The fragment is put there for the NEGATIVE pair: normal (0, 1, 0) under light direction (0, -1, 0) gives ndl = -1 exactly,
    bias = 1 - ndl = 2, so negCurrentDepth = -exp(-40 (pz + 0.0001 * 2)) is y2 at pz = z2 - 0.0002.  The positive pair then sits at exp(40 (pz + 0.003 *
    2)) = x2 e^0.232 = 1.26 x2, FURTHER above its mean than x2 is, so its bound is below 1 - p (0.42 for p = 0.25, 0.30 for p = 0.5): the factor is
    1 - max(positive, negative) = 1 - (1 - p) = p.  To 1e-5 relative, on the float64 restatement and on the C oracle (a rounding of pz moves y2 by
    40 dz of itself, and y2 is 2e-9 against y2 - y1 = 6e-6; the moments' float32 storage moves the variance by 1e-7 of itself)."""
    case = csm_cases.two_level(p)
    for shade in (f64_shade, c_shade):
        factor = shadow_factor(shade, case)
        np.testing.assert_allclose(factor, p, rtol=1e-5, atol=0.0)


@pytest.mark.parametrize("name", list(csm_cases.MISSING))
def test_missing_maps_give_factor_one_on_the_c_oracle(name):
    """"no map bound => shadow factor 1" (include/sailor_hip.h): with cascade k's map absent the pixels of cascade k are, bit for bit, those of the frame
    shaded with no shadow maps at all; the other cascades' pixels are those of the frame with all four maps."""
    case = csm_cases.build(name)
    full = csm_cases.build("size-16x8")
    f = case.frame
    got = csm_cases.c_oracle(f)
    none = csm_cases.c_oracle(f, csm=False)
    absent = np.isin(case.notes["cascade"], csm_cases.MISSING[name])
    assert absent.any() and np.array_equal(got[absent].view(np.uint32), none[absent].view(np.uint32))
    with_all = csm_cases.c_oracle(full.frame)
    assert np.array_equal(got[~absent].view(np.uint32), with_all[~absent].view(np.uint32))
    assert (with_all[absent] != none[absent]).any(), "the maps must change the picture where they are bound"
