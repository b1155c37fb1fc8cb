"""The indirect surface draw without a GPU: the entry point is exported and the version says so; the restatement of the indirect pass (tests/indirect_ref.py:
every draw alone with its capacity-based primBase, the maximum of the keys) decodes to the owners of the sequential direct pass over the survivors for every
case of tests/indirect_cases.py, with and without a prepass and in bands; every case reaches what it was built to reach; the instances of the chain scenes are
all decided in float64 and the C oracle's survivor counts are the ones written in the case table."""
import numpy as np
import pytest

import indirect_cases as cases
import indirect_ref as iref
from oracle import oracle, oracle_f64
from sailor_amd import _lib, host


def test_the_entry_point_is_exported_and_the_version_is_9():
    lib = _lib.load()
    assert hasattr(lib, "sailor_hip_surface_draw_indirect")
    assert len(_lib.SIGNATURES["sailor_hip_surface_draw_indirect"][1]) == 16
    assert lib.sailor_hip_version() >= 9


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: iref.expected(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


def test_rule_3_on_its_edges():
    ind = lambda capacity, count, first: dict(capacity=capacity, count=count, first=first, records=None)
    assert iref.drawn(ind(24, 5, 0), 26) == 5 and iref.drawn(ind(24, 30, 0), 26) == 24 and iref.drawn(ind(24, 24, 20), 26) == 6
    assert iref.drawn(ind(24, 5, 26), 26) == 0 and iref.drawn(ind(24, 5, 25), 26) == 1 and iref.drawn(ind(24, 2 ** 32 - 1, 2 ** 32 - 1), 26) == 0
    assert iref.drawn(ind(0, 5, 0), 26) == 0 and iref.drawn(dict(capacity=9, count=9, first=3, records=4), 26) == 1


@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_indirect_pass_decodes_to_the_direct_pass_over_the_survivors(scenes, rendered, name):
    s, want = scenes[name], rendered[name]
    direct = iref.decode(want["keys"], iref.prim_table(s, "survivors"))
    assert cases.CASES[name][1](want, direct, s), f"{name} does not reach what it was built for"
    got = iref.decode(iref.render_keys(s), iref.prim_table(s, "capacity"))
    assert iref.same_owners(got, direct), name
    np.testing.assert_array_equal(direct["slot"] >= 0, want["covered"])
    # no draw reaches the slack, and the direct pass over the survivors never names a record at or beyond `records`
    for k, d in enumerate(iref.survivors(s)["draws"]):
        if d["instance_ids"] is None and d["num_drawn"]:
            assert d["first_instance"] + d["num_drawn"] <= s["records"], (name, k)


def test_behind_a_prepass_and_in_bands(scenes):
    for name in cases.BAND_CASES:
        s = scenes[name]
        pre = cases.prepass(iref.survivors(s))
        want = iref.expected(s, prepass=pre)
        assert iref.same_owners(iref.decode(iref.render_keys(s, prepass=pre), iref.prim_table(s, "capacity")),
                                iref.decode(want["keys"], iref.prim_table(s, "survivors"))), name
        np.testing.assert_array_equal(want["depth"].view(np.uint32), pre.view(np.uint32), err_msg=f"{name}: the pass behind its own prepass changes no depth")
        parts = []
        for rank in reversed(range(2)):
            band = host.band_for_rank(s["W"], s["H"], rank, 2)
            rows = (band.fbRowBegin, band.fbRowBegin + band.fbRowCount)
            parts.append(iref.render_keys(s, rows=rows))
        assert iref.same_owners(iref.decode(np.concatenate(parts), iref.prim_table(s, "capacity")),
                                iref.decode(iref.expected(s)["keys"], iref.prim_table(s, "survivors"))), name


def test_a_partially_counted_draw_changes_the_low_words_behind_it(scenes, rendered):
    """rule 5: the next draw's primBase advances by the capacity, so the backdrop's keys differ from the direct pass's in the low word and in nothing else"""
    s, want = scenes["boxes_5_of_24"], rendered["boxes_5_of_24"]
    keys = iref.render_keys(s)
    assert iref.prim_table(s, "capacity")[1][0] == 24 * 24 and iref.prim_table(s, "survivors")[1][0] == 5 * 24
    behind = iref.decode(want["keys"], iref.prim_table(s, "survivors"))["slot"] == 1
    assert behind.sum() > 1000
    np.testing.assert_array_equal(keys[behind] - want["keys"][behind], np.uint64((24 - 5) * 24))
    np.testing.assert_array_equal(keys[~behind], want["keys"][~behind])


@pytest.mark.parametrize("name", list(cases.CHAINS))
def test_chain_scenes_are_decided_in_float64_and_the_counts_are_the_tables(name):
    build, counts = cases.CHAINS[name]
    c = build()
    s = c["scene"]
    n = s["records"]
    hiz = None
    if "hiz" in c:   # the pyramid of the wall's depth, by the C oracle over the restatement's depth
        wall = dict(iref.survivors(s), draws=iref.survivors(s)["draws"][:1])
        w, h, levels = c["hiz"]
        hiz = (oracle.hiz_build(iref.renderer(wall)(wall)["depth"], w, h, levels), w, h, levels)
    f64 = oracle_f64.mesh_cull_flags(bytes(c["frame"]), s["instances"][:n], hiz)
    assert f64["decided"].all(), (name, np.nonzero(~f64["decided"])[0])
    after, got = cases.chain_after_cull(c, hiz)
    assert got == counts, (name, got)
    for k, b in enumerate(c["batches"]):
        assert int((~f64["culled"][b[4]: b[4] + b[1]]).sum()) == counts[k], (name, k)
    # the culled frame is the un-culled one: depth, planes and coverage (every culled instance is invisible)
    culled, whole = iref.expected(after), iref.expected(s)
    if hiz is None:
        np.testing.assert_array_equal(culled["depth"].view(np.uint32), whole["depth"].view(np.uint32))
        np.testing.assert_array_equal(culled["covered"], whole["covered"])
        np.testing.assert_array_equal(culled["planes"].view(np.uint32), whole["planes"].view(np.uint32))
        assert culled["covered"].sum() > 500
    else:         # the frame is the wall's
        wall_only = iref.renderer(wall)(wall)
        np.testing.assert_array_equal(culled["keys"], wall_only["keys"])
        np.testing.assert_array_equal(whole["keys"], wall_only["keys"])
        assert wall_only["covered"].all()
