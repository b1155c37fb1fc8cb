"""The Masked queue without a GPU: tests/masked_ref.py (the sequential float32 restatement the kernels of sailor_amd/csrc/surface_masked.hip are held to) against
the counts every case of tests/masked_cases.py was built to reach, against tests/surface_ref.py where no draw carries ALPHA_CUTOUT, against its screen-linear
mutant, against its own float64 twin of the alpha, and against the golden file."""
import numpy as np
import pytest

import masked_cases as cases
import masked_ref
import surface_cases
import surface_ref as ref
from make_masked_golden import PATH as GOLDEN, masked_golden_scene

# the largest |alpha32 - alpha64| over every case and every soup, as measured (recorded in DESIGN.md, "The Masked queue"); the margin of the decision test is
# 4 x this, the project's convention: headroom for a different but legal rounding order
MEASURED_ALPHA_ERROR = 3.37e-6
MARGIN = 4 * MEASURED_ALPHA_ERROR


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: masked_ref.render(s) for name, s in scenes.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_reaches_what_it_was_built_for(scenes, rendered, name):
    assert cases.CASES[name][1](rendered[name], scenes[name]), rendered[name]["stats"]


def test_the_soups_reach_discards_survivors_and_cuts(rendered):
    total = dict(tested=0, discarded=0, cut_one=0, cut_two=0, overwritten=0, beyond_table=0)
    survivors = 0
    for seed in range(cases.NUM_SOUPS):
        st = rendered[f"masked_soup_{seed}"]["stats"]
        for k in total:
            total[k] += st[k]
        survivors += st["tested"] - st["discarded"]
    assert all(v > 0 for v in total.values()) and survivors > 1000, (total, survivors)


def test_without_a_cutout_draw_the_restatement_is_surface_refs_bit_for_bit():
    for name in ("multiple_draws", "near_plane", "instance_indirection", "texture_2x3_srgb", "tie_two_draws", "triangle_larger_than_the_frame"):
        s = surface_cases.CASES[name][0]()
        pre = surface_cases.prepass_depth(s)
        for prepass, rows in ((None, None), (pre, None), (None, (3, 17))):
            got, want = masked_ref.render(s, prepass=prepass, rows=rows), ref.render(s, prepass=prepass, rows=rows)
            for k in ("keys", "depth", "covered"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")
            assert ref.same_bits_or_class(got["planes"], want["planes"]).all(), name
            assert got["stats"]["tested"] == 0 and {k: v for k, v in want["stats"].items()} == {k: got["stats"][k] for k in want["stats"]}, name
    for seed in (0, 7):
        s = surface_cases.random_soup(seed)
        np.testing.assert_array_equal(masked_ref.render(s)["keys"], ref.render(s)["keys"])


def test_the_screen_linear_mutant_differs_on_the_oblique_quad(scenes, rendered):
    s = scenes["colour_alpha_oblique"]
    mutant = masked_ref.render(s, perspective=False)
    assert (mutant["covered"] != rendered["colour_alpha_oblique"]["covered"]).sum() > 50
    assert not np.array_equal(mutant["keys"], rendered["colour_alpha_oblique"]["keys"])


def test_every_pixel_a_cutout_draw_owns_holds_an_alpha_that_survives(rendered):
    owned = 0
    for name, r in rendered.items():
        a = r["planes"][0][..., 3][r["cutout"]]
        assert ((a >= np.float32(0.5)) | np.isnan(a)).all(), name
        assert r["covered"][r["cutout"]].all(), name
        owned += a.size
    assert owned > 5000


def test_discarded_fragments_leave_the_depth_alone(scenes, rendered):
    for name in ("discarded_in_front", "threshold_bytes", "no_texels_and_beyond_table", "checker_over_opaque"):
        r = rendered[name]
        assert ((r["depth"] > 0) == r["covered"]).all(), name   # (no prepass: depth only where something survived)


def test_fp32_and_float64_discard_decisions_agree_outside_the_margin(rendered):
    worst, tested, near = 0.0, 0, 0
    for name, r in rendered.items():
        a32, a64 = r["alpha32"], r["alpha64"]
        assert a32.size == a64.size == r["stats"]["tested"], name
        assert np.array_equal(np.isnan(a32), np.isnan(a64)) and np.array_equal(np.isposinf(a32), np.isposinf(a64)), name
        fin = np.isfinite(a32) & np.isfinite(a64)
        if fin.any():
            e = float(np.abs(a32[fin].astype(np.float64) - a64[fin]).max())
            print(f"{name}: {a32.size} tested, max |alpha32 - alpha64| = {e:.3g}")
            worst = max(worst, e)
        d32, d64 = a32 < np.float32(0.5), a64 < 0.5
        if name in cases.EXACT_THRESHOLD_CASES:
            assert np.array_equal(d32, d64), f"{name}: the exact-threshold cases are compared without a margin"
            continue
        close = np.abs(a64 - 0.5) <= MARGIN
        assert np.array_equal(d32[~close], d64[~close]), f"{name}: {(d32 != d64)[~close].sum()} decisions differ outside the margin"
        tested += a32.size
        near += int(close.sum())
    print(f"max |alpha32 - alpha64| over everything: {worst:.3g}; {near} of {tested} tested fragments within the margin {MARGIN:.3g}")
    assert worst <= MEASURED_ALPHA_ERROR, worst
    assert tested > 10000 and near * 100 <= tested, (near, tested)   # a condition on the scenes, not a measurement: at most 1 in 100


def test_masked_prepass_depth_keeps_the_opaque_depth_in_the_holes(scenes):
    s = scenes["checker_over_opaque"]
    opaque = cases.opaque_prepass(s)
    full = cases.full_prepass(s)
    r = masked_ref.render(s)
    np.testing.assert_array_equal(full.view(np.uint32), r["depth"].view(np.uint32))
    holes = ~r["cutout"] & (opaque > 0)
    assert holes[4:20, 6:33].sum() > 100
    np.testing.assert_array_equal(full[holes].view(np.uint32), opaque[holes].view(np.uint32))
    behind = masked_ref.render(s, prepass=full)   # a RenderScene pass begun from it covers the same pixels
    np.testing.assert_array_equal(behind["covered"], r["covered"])
    np.testing.assert_array_equal(behind["keys"], r["keys"])


def test_golden_file():
    g = np.load(GOLDEN)
    name = cases.GOLDEN_CASE
    s = masked_golden_scene(g)
    assert [d["alpha_cutout"] for d in s["draws"]] == [False, True]
    r = masked_ref.render(s)
    np.testing.assert_array_equal(r["keys"], g[f"{name}.keys"])
    assert ref.same_bits_or_class(r["planes"], g[f"{name}.planes"]).all()
    assert GOLDEN.stat().st_size < 64 * 1024
