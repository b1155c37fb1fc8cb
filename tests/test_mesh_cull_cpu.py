"""The instance visibility path on the CPU: the C oracle (oracle/sailor_oracle.c: mesh_cull_flags, occlusion_culling, hiz_fetch_min, oracle_hiz_build,
the step-3 compaction) against the float64 restatement written from the shader text (oracle/oracle_f64.py: mesh_cull_flags, hiz_fetch_min, hiz_build,
compact_partition) on the placed cases of tests/mesh_cull_cases.py.  The kernels run the same cases in tests/test_mesh_cull_edges_gpu.py."""
import numpy as np
import pytest

import mesh_cull_cases as cases
from oracle import oracle, oracle_f64

SCENE_CAP = 0.01   # at most 1 % of a scene-* case's instances may be left undecided by the float64 bound: a condition on the scene, not a measurement


@pytest.mark.parametrize("name", cases.NAMES)
def test_oracle_flags_agree_with_float64_wherever_decided(name):
    """The agreement test.  Per case: the C oracle's flag equals the float64 reference's wherever every decision on the path the reference takes is
    beyond its fp32 bound; exact-* cases are decided on every instance (ties included); a scene-* case leaves at most 1 % undecided; every group of
    a flip-* case holds both outcomes in the C oracle's own flags.

    Measured: undecided / instances -- exact-* 0 of 5..14; flip-plane-tie-zero-radius 24 / 24 (the bound cannot know that the two products cancel: the
    tie is asserted on the flags in test_plane_tie_is_kept); flip-planes-identity 392 / 440 and flip-planes-camera 375 / 440 (the 49 adjacent floats of
    each group lie inside the bound of the plane normals, the six farther ones are decided); flip-level-16x16 137 / 516, flip-level-camera-24x10
    158 / 516; footprint-16x16 2 / 33, footprint-24x10 9 / 33 (texel-centre hits through an inexact chain, the NaN centres); scene-* 0 / 2048 each.
    The C oracle and the reference differ inside the undecided set on 4, 2, 7 and 7 instances of the flip-planes-* and flip-level-* cases and nowhere
    else.

    Mutants of the C oracle (a scratch copy, one change each) and the tests of this file that fail on them:
      depthSphere <= depth            this test [exact-depth-tie], test_exact_ties_of_the_issue
      C.z <= r + znear                this test [exact-gate, footprint-16x16, footprint-24x10], test_footprints_under_the_one_texel_probe [both],
                                      test_exact_ties_of_the_issue
      dot - w <= -radius              test_plane_tie_is_kept, test_case_groups_hold_both_outcomes [flip-plane-tie-zero-radius]
      cz - r >= zFar                  this test [exact-zrange], test_exact_ties_of_the_issue
      useX1 always true               test_footprints_under_the_one_texel_probe [footprint-24x10], test_hiz_oracle_equals_float64_where_the_footprints_agree
                                      [11 of the 20 shapes], test_hiz_own_chain_agrees_outside_the_convention_texels
      level e + 1 before the clamp    this test [flip-level-16x16, flip-level-camera-24x10, scene-*], test_case_groups_hold_both_outcomes [flip-level-*],
                                      test_footprints_under_the_one_texel_probe [both]
      max(width, height) -> width     this test [scene-*], test_footprints_under_the_one_texel_probe [footprint-16x16]
      second texel floor(x + 1.0f)    test_hiz_oracle_equals_float64_where_the_footprints_agree [one-column] -- the fetch as it stood before these
                                      tests: for x = -2^-25 the sum rounds to 1.0f and texel 1, which is outside the footprint, was read"""
    case, ref = cases.build(name), cases.reference(name)
    got = cases.oracle_flags(name) == 1
    dec = ref["decided"]
    differ = got != ref["culled"]
    print(f"{name}: instances {len(got)}, undecided {int((~dec).sum())}, oracle != float64 {int(differ.sum())} (decided among them {int((differ & dec).sum())})")
    assert not (differ & dec).any(), np.nonzero(differ & dec)[0]
    if case.exact:
        assert dec.all(), np.nonzero(~dec)[0]
    if name.startswith("scene-"):
        assert (~dec).sum() <= SCENE_CAP * len(got)
        assert 0 < got.sum() < len(got)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.build(n).both_outcomes])
def test_case_groups_hold_both_outcomes(name):
    """a flip-* group steps one input over adjacent floats: the flip has to happen inside it, in the C oracle's flags and in the reference's"""
    case, ref = cases.build(name), cases.reference(name)
    got = cases.oracle_flags(name)
    for g in case.both_outcomes:
        assert got[g].min() == 0 and got[g].max() == 1, g
        assert ref["culled"][g].any() and not ref["culled"][g].all(), g


def test_plane_tie_is_kept():
    """dot(n, c) - w < -radius with both sides 0 (a sphere of radius 0 whose centre lies in a side plane, where the two products of the dot cancel
    exactly): not culled; the float farther out is"""
    case, got = cases.build("flip-plane-tie-zero-radius"), cases.oracle_flags("flip-plane-tie-zero-radius")
    for g in case.both_outcomes:
        tie, away = got[g][1], got[g][0] if case.instances["sphereBounds"][g][0, :2].sum() < 0 else got[g][2]
        assert (tie, away) == (0, 1), (g, got[g])


@pytest.mark.parametrize("name", cases.PROBE_NAMES)
def test_footprints_under_the_one_texel_probe(name):
    """The flag hides level and footprint; the probe shows them: with the pyramid at 2.0 and one texel at 0.0 an instance that passes the frustum test
    and the gate stays unculled exactly when its fetch reads that texel.  The set of probes an instance survives, from the C oracle, equals the
    float64 footprint wherever frustum, gate, level and both axes are decided; the instances placed on texel centres have the texel count their
    level's geometry gives."""
    case, ref = cases.build(name), cases.reference(name)
    got, want = cases.oracle_probe_survivors(name), cases.reference_probe_survivors(name)
    dec = ref["frustum_decided"] & ref["gate_decided"] & ref["level_decided"] & ref["footprint_decided"]
    bad = (got != want).any(0)
    print(f"{name}: {got.shape[0]} probes x {got.shape[1]} instances, footprint undecided {int((~dec).sum())}, differing {int(bad.sum())}")
    assert not (bad & dec).any(), np.nonzero(bad & dec)[0]
    sizes = got.sum(0)
    for i, k in case.texels.items():
        assert sizes[i] == k, (i, sizes[i], k)
    # the issue's two probes, checked to the texel
    if name == "footprint-16x16":
        assert set(np.nonzero(got[:, 0])[0]) == {336, 337, 338, 339} and set(np.nonzero(got[:, 1])[0]) == {127, 143}


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_coverage(name):
    """every count a case names is non-zero on the reference's own decisions"""
    cov = cases.coverage(name)
    missing = [k for k in cases.build(name).expect if cov[k] == 0]
    assert not missing, (missing, cov)


def test_the_cases_together_reach_every_key():
    total = {k: 0 for k in cases.COVERAGE_KEYS}
    for name in cases.NAMES:
        for k, v in cases.coverage(name).items():
            total[k] += v
    print(total)
    assert not [k for k, v in total.items() if v == 0]


def test_exact_ties_of_the_issue():
    """the ties stated in the issue, one by one, on the C oracle and the reference (identity view, fov 90, 64 x 64 viewport, near 1)"""
    fr = cases.identity_frame()
    def flags(centre, r, value):
        inst = cases.records([centre], r)
        hiz = cases.constant_pyramid(16, 16, 5, value)
        ref = oracle_f64.mesh_cull_flags(bytes(fr), inst, hiz)
        assert ref["decided"][0]
        return int(oracle.mesh_cull_occlusion(fr, inst, *hiz)["isCulled"][0]), int(ref["culled"][0])
    below4 = float(cases.step_floats(4.0, [-1])[0])
    assert flags((0, 0, -4.0), 3.0, 2.0) == (1, 1)                   # C.z == r + znear: the gate passes, occluded by 2.0
    assert flags((0, 0, -below4), 3.0, 2.0) == (0, 0)                # the float below: the gate returns false
    assert flags((0, 0, -7.0), 3.0, 0.25) == (0, 0)                  # depthSphere == depth: not occluded
    assert flags((0, 0, -7.0), 3.0, cases.step_floats(0.25, [1])[0]) == (1, 1)
    assert flags((0, 0, -20003.0), 3.0, 0.0) == (0, 0) and flags((0, 0, -20004.0), 3.0, 0.0) == (1, 1)     # cz - r == 20000 kept, 20001 culled
    assert flags((0, 0, 2.0), 3.0, 0.0) == (0, 0) and flags((0, 0, 2.5), 3.0, 0.0) == (1, 1)               # cz + r == 1 kept, 0.5 culled


def test_level_selection_at_the_clamps():
    """floor(log2(m)) clamped to the chain, on the reference: m < 1, m <= 0 and NaN give level 0, m >= 2^levels and +Inf the top level"""
    ref = cases.reference("footprint-16x16")
    with np.errstate(invalid="ignore"):
        gate, m, level = ref["gate"], ref["m"], ref["level"]
        assert (level[gate & (m < 1)] == 0).all() and (level[gate & np.isnan(m)] == 0).all() and (level[gate & (m >= 32)] == 4).all()
        assert (gate & (m > 0) & (m < 1)).any() and (gate & (m <= 0)).any() and (gate & np.isnan(m)).any() and (gate & (m >= 32)).any()
        assert not ref["decided"][gate & np.isnan(m)].any()                 # what fp32 leaves to the implementation is not called decided


def test_fetch_reference_footprints():
    """oracle_f64.hiz_fetch_min on a 4 x 3 level: texel centres (one texel), texel corners (four), clamped edges and corners with uv outside [0, 1],
    an infinite coordinate (the edge texel), a NaN one (not decided)"""
    tex = np.arange(12, dtype=np.float64).reshape(3, 4) + 1.0
    f = oracle_f64.hiz_fetch_min(tex, [0.375, 0.5, 0.375, -0.5, 1.5, 1.5, np.inf, np.nan, 0.5], [0.5, 0.5, 1.0 / 3.0, 0.5, 0.5, -2.0, 0.5, 0.5, 7.0])
    sets = oracle_f64.footprint_sets(f["texels"])
    assert sets[0] == {5} and sets[1] == {5, 6} and sets[2] == {1, 5} and sets[3] == {4} and sets[4] == {7} and sets[5] == {3} and sets[6] == {7}
    assert sets[8] == {9, 10}
    assert list(f["value"][:7]) == [6.0, 6.0, 2.0, 5.0, 8.0, 4.0, 8.0]
    assert f["decided"][[0, 1, 3, 4, 5, 6, 8]].all() and not f["decided"][7]
    assert f["decided"][2]
    # the same centre hit with coordinates that carry a rounding: which side of the texel border the fp32 value falls is not decided
    g = oracle_f64.hiz_fetch_min(tex, [0.375], [0.5], eu=0.375)
    assert oracle_f64.footprint_sets(g["texels"])[0] == {5} and not g["decided"][0]


# ---- Hi-Z pyramid ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.HIZ_NAMES)
def test_hiz_oracle_equals_float64_where_the_footprints_agree(name):
    """oracle_hiz_build, level by level, against the float64 downscale of the SAME source level with sample positions in exact rational arithmetic.
    Where the fp32 evaluation of (i + 0.5) / dst * src - 0.5 selects the exact footprint the values are equal; the other texels ("sampler-convention
    texels": the canonical fetch counts a neighbour whenever the fp32 fraction is not exactly 0, a hardware sampler would quantise it to 0) are
    counted per level as (columns, rows) and equal the pinned counts: 25 of the 960 columns of the shipped pyramid's own 960 -> 960 step, 2 of 131 ->
    131, none for powers of two, 48 -> 16, 36 -> 12, 96 -> 96 and every 2:1 step.  A texel whose footprint holds a NaN is compared by class only: the
    oracle's `t < m ? t : m` keeps a leading NaN and drops a later one, and the sampler's rule is not specified."""
    raw, W, H, levels, counts = cases.hiz_source(name)
    got = cases.hiz_oracle(name)
    ref = oracle_f64.hiz_build(raw, W, H, levels, given=got)
    print(f"{name}: convention (columns, rows) per level {ref['convention']}, texels outside agreement {int((~ref['agree']).sum())} of {got.size}")
    if counts is not None:
        assert ref["convention"] == counts
    assert ref["agree"].mean() >= 0.9                                # the comparison below is not vacuous
    clean = ref["agree"] & ~ref["nan"]
    np.testing.assert_array_equal(got[clean].astype(np.float64), ref["pyramid"][clean])
    dirty = ref["agree"] & ref["nan"]
    g = got[dirty].astype(np.float64)
    assert (np.isnan(g) | (g == ref["pyramid"][dirty]) | (np.isnan(ref["pyramid"][dirty]))).all()
    if name == "source-nan":
        assert dirty.any() and np.isnan(g).any() and (~np.isnan(g)).any()
    if name == "source-inf":
        assert np.isinf(got).any() and not np.isinf(got[-1:]).all() or np.isinf(raw).all()
    if name == "source-zeros":
        assert (got == 0).any()
    # the conservative direction of the convention texels: a neighbour more can only lower the minimum (a farther depth)
    other = ~ref["agree"] & ~ref["nan"]
    assert (got[other].astype(np.float64) <= ref["pyramid"][other]).all()


def test_sampler_convention_columns_of_single_steps():
    """the count behind the pinned figures, on the two axis evaluations alone (no image): exact rational position against the fp32 chain"""
    def differ(src, dst):
        a, b = oracle_f64._hiz_axis_exact(src, dst), oracle_f64._hiz_axis_fp32(src, dst)
        return int(((a[0] != b[0]) | (a[1] != b[1])).sum())
    assert differ(960, 960) == 25 and differ(131, 131) == 2
    for src, dst in [(96, 96), (48, 16), (36, 12), (64, 64), (1024, 1024), (4096, 4096), (540, 960)] + [(2 * d, d) for d in (1, 3, 5, 48, 65, 131, 480, 960)]:
        assert differ(src, dst) == 0, (src, dst)


def test_hiz_own_chain_agrees_outside_the_convention_texels():
    """the reference's own chain (every level from ITS level below): equal to the oracle wherever no convention texel lies under the texel"""
    raw, W, H, levels, _ = cases.hiz_source("same-131")
    ref = oracle_f64.hiz_build(raw, W, H, levels)
    got = cases.hiz_oracle("same-131")
    assert 0 < (~ref["agree"]).sum() < 0.05 * got.size
    np.testing.assert_array_equal(got[ref["agree"]].astype(np.float64), ref["pyramid"][ref["agree"]])


# ---- compaction --------------------------------------------------------------------------------------------------------------------------------
def _check_compaction(inst, batches):
    cam = cases.compact_camera()
    want_words, want_batches = cases.compact_expected(cam.frame, inst, batches)
    got_i, got_b = oracle.mesh_cull_compact(cam.frame, inst, len(inst), 0, batches)
    np.testing.assert_array_equal(got_b, want_batches)
    np.testing.assert_array_equal(got_i.view(np.uint32).reshape(-1, 24), want_words)
    return got_i, got_b


@pytest.mark.parametrize("count", cases.COMPACT_COUNTS)
def test_compaction_oracle_is_the_partition_on_every_pattern(count):
    for pattern in cases.COMPACT_PATTERNS:
        inst, batches = cases.compact_single(count, pattern)
        _, got_b = _check_compaction(inst, batches)
        assert got_b[0, 1] == cases.keep_pattern(pattern, count).sum(), pattern     # the keep pattern is the one the positions were meant to give


@pytest.mark.parametrize("num_batches", cases.COMPACT_BATCH_NUMBERS)
def test_compaction_oracle_many_batches(num_batches):
    inst, batches = cases.compact_many(num_batches)
    assert len(inst) < 70000
    _check_compaction(inst, batches)


def test_compaction_oracle_gaps_and_order():
    inst, batches = cases.compact_gaps()
    got_i, _ = _check_compaction(inst, batches)
    owned = np.zeros(len(inst), bool)
    for f, c in zip(batches[:, 4], batches[:, 1]):
        owned[f:f + c] = True
    w0, w1 = inst.view(np.uint32).reshape(-1, 24), got_i.view(np.uint32).reshape(-1, 24)
    keep = np.ones(24, bool); keep[21] = False
    np.testing.assert_array_equal(w1[~owned][:, keep], w0[~owned][:, keep])          # a gap record: byte for byte apart from the flag
    assert (w1[~owned][:, 21] <= 1).all() and (~owned).sum() > 1000
