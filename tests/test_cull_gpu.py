"""K0 + K1 on the constructed scenes of tests/cull_cases.py (GPU): every path of sailor_amd/csrc/light_cull.hip -- the plane-test masks, the brute-force
walk, the interval masks, tile-row bands with and without the band's own light selection, the prepared-lights entries, the deferred pack, the raw-depth
form -- against the C oracle's lists, bit for bit, where spheres touch tile planes, band planes and depth bounds to the float.  What each case reaches
and that the references agree on it is tests/test_cull_cpu.py's business; here the structural cases also assert that they took their path."""
import numpy as np
import pytest
import torch

import cull_cases as cc
from sailor_amd import _lib, host
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, upload_lights
from test_light_cull_gpu import assert_lists_equal

pytestmark = pytest.mark.gpu

CASES = list(cc.CASES)


class Scene:
    """a case on the device: the lights uploaded once, the depth rows of any band"""

    def __init__(self, ctx, name):
        self.ctx, self.name, self.c = ctx, name, cc.build(name)
        self.W, self.H = self.c.size
        self.N = len(self.c.lights)
        self.lights = upload_lights(self.c.lights, ctx.device)
        self.geo = cc.Geo(self.c.cam)

    def band(self, rank_of):
        return None if rank_of is None else host.band_for_rank(self.W, self.H, *rank_of)

    def cull(self, flags=_lib.CULL_DEFAULT, rank_of=None, raw=False, prepared=None, **kw):
        """-> (the ForwardPlus after the cull, the names of the kernels the cull launched)"""
        fp = ForwardPlus(self.ctx, self.W, self.H, self.N, band=self.band(rank_of), prepared=prepared)
        b = fp.band
        img = self.c.raw_depth if raw else self.c.depth
        d = torch.from_numpy(np.ascontiguousarray(img[b.fbRowBegin:b.fbRowBegin + b.fbRowCount])).to(self.ctx.device)
        names = self.ctx.launches_of(lambda: fp.cull(self.c.cam.frame, self.lights, self.N, d, flags | (_lib.CULL_RAW_DEPTH if raw else 0), **kw))
        return fp, names

    def ref(self, rank_of=None):
        g, i, _ = cc.c_lists(self.name, rank_of)
        return g, i


@pytest.fixture(scope="module")
def scene(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                      # one case's buffers at a time (the tests of a case run next to each other: see the parametrisation)
            cache[name] = Scene(ctx, name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_whole_frame_paths(scene, name):
    """CULL_DEFAULT, CULL_BRUTE_FORCE, CULL_INTERVAL_MASKS (and CULL_RAW_DEPTH on the reversed-Z image) == the C oracle; the default path is the
    brute-force walk exactly for the cases below 512 lights or outside the `sane` perspective gate, the wide group lists from 4 096 mask words
    on, and the counted groups hold exactly the constructed number of candidates (CAPG + 1: the group overflows)."""
    s = scene(name)
    g, i = s.ref()
    for flags in (_lib.CULL_DEFAULT, _lib.CULL_BRUTE_FORCE, _lib.CULL_INTERVAL_MASKS):
        fp, names = s.cull(flags)
        assert_lists_equal(fp.lists_to_host(), g, i)
        if flags == _lib.CULL_DEFAULT:
            assert any("brute" in n for n in names) == (name in cc.BRUTE), names
            assert ("k1_group_lists_wide" in names) == (name in cc.HUGE), names
            if name not in cc.BRUTE and name not in cc.HUGE:
                assert names == ["k01_prepare", "k1_group_lists", "k1_tile_cull", "k1_pack"], names
            if "group_max" in s.c.notes:
                diag, cov = fp.cull_diagnostics(s.N), cc.coverage(name)
                assert diag["group_list_max"] == cov["group_max_frame"] and diag["groups_overflowed"] == cov["groups_over_capg_frame"], (diag, cov)
                assert diag["groups_overflowed"] == (1 if s.c.notes["group_max"] > cc.CAPG else 0)
                assert s.c.notes["group_max"] > cc.CAPG or diag["group_list_max"] == s.c.notes["group_max"]
        elif flags == _lib.CULL_BRUTE_FORCE:
            assert any("brute" in n for n in names), names
    if s.c.raw_depth is not None:
        for flags in (_lib.CULL_DEFAULT, _lib.CULL_BRUTE_FORCE):
            fp, _ = s.cull(flags, raw=True)
            assert_lists_equal(fp.lists_to_host(), g, i)


@pytest.mark.parametrize("name", CASES)
def test_bands_with_and_without_their_own_light_selection(scene, name):
    """The bands of 2 and 3 ranks under CULL_BAND_SELECT and CULL_NO_BAND_SELECT == the C oracle's lists of those tile rows.  Where the selection ran
    (k0_band_count is among the launches), the band's light set holds EVERY light that the fp32 table accepts for any tile of the band, in
    ascending order -- k0_band_count held to the table directly, independent of the 196-candidate cut -- and on the first band of two ranks the
    counted group holds the constructed number of candidates."""
    s = scene(name)
    ok32 = cc.tables(name)[0]
    for rank_of in cc.RANKS:
        r0, r1 = s.geo.band_rows(rank_of)
        if r0 == r1:
            continue
        g, i = s.ref(rank_of)
        for flags in (_lib.CULL_BAND_SELECT, _lib.CULL_NO_BAND_SELECT):
            fp, names = s.cull(flags, rank_of)
            assert_lists_equal(fp.lists_to_host(), g, i)
            if flags == _lib.CULL_BAND_SELECT:
                assert ("k0_band_count" in names) == (name not in cc.BRUTE), names
            else:
                assert "k0_band_count" not in names, names
            if "k0_band_count" in names:
                m, lm = fp.band_selection(s.N)
                assert len(lm) == m and (np.diff(lm.astype(np.int64)) > 0).all()
                need = np.nonzero(ok32[r0 * s.geo.Tx: r1 * s.geo.Tx].any(0))[0]
                missing = np.setdiff1d(need, lm)
                assert len(missing) == 0, f"{name} {rank_of}: the band selection dropped lights {missing[:8].tolist()} that a tile of the band lists"
            elif "group_max" in s.c.notes and rank_of == (0, 2) and name not in cc.BRUTE:
                diag, cov = fp.cull_diagnostics(s.N), cc.coverage(name)
                assert diag["group_list_max"] == cov["group_max_rank0of2"] and diag["groups_overflowed"] == cov["groups_over_capg_rank0of2"], (diag, cov)


@pytest.mark.parametrize("name", CASES)
def test_prepared_lights_and_the_deferred_pack(scene, name):
    """The prepared-lights entry (the 20-byte views derived beforehand, and derived inside the cull with prepare_lights=True -- also behind a band's
    selection) and the per-tile slots after defer_pack=True, then pack(): the same lists."""
    s = scene(name)
    ctx = s.ctx
    g, i = s.ref()
    ready = PreparedLights(ctx, s.lights, s.N)
    fp, _ = s.cull(prepared=ready)
    assert_lists_equal(fp.lists_to_host(), g, i)
    mine = PreparedLights(ctx, s.lights, 0, capacity=s.N)
    mine.buffer.fill_(0x5A)
    fp, _ = s.cull(prepared=mine, prepare_lights=True)
    assert_lists_equal(fp.lists_to_host(), g, i)
    ctx.synchronize()
    for a, b in zip(mine.views()[:2], ready.views()[:2]):
        np.testing.assert_array_equal(a.cpu().numpy()[: s.N].view(np.uint32), b.cpu().numpy()[: s.N].view(np.uint32))
    rank_of = (1, 2)
    if s.geo.band_rows(rank_of)[0] != s.geo.band_rows(rank_of)[1]:
        bg, bi = s.ref(rank_of)
        mine.buffer.fill_(0x5A)
        fp, _ = s.cull(_lib.CULL_BAND_SELECT, rank_of, prepared=mine, prepare_lights=True)
        assert_lists_equal(fp.lists_to_host(), bg, bi)
    # the deferred pack
    fp = ForwardPlus(ctx, s.W, s.H, s.N)
    d = torch.from_numpy(np.ascontiguousarray(s.c.depth)).to(ctx.device)
    fp.grid.fill_(-7); fp.culled.fill_(-7)
    fp.cull(s.c.cam.frame, s.lights, s.N, d, defer_pack=True)
    ctx.synchronize()
    assert (fp.grid == -7).all() and (fp.culled == -7).all(), "a deferred cull does not write the canonical buffers"
    base = fp.workspace.data_ptr()
    T = fp.band_tiles
    num = fp.workspace[fp.tile_num - base: fp.tile_num - base + 4 * T].view(torch.int32).cpu().numpy().view(np.uint32)
    lists = fp.workspace[fp.tile_lists - base: fp.tile_lists - base + 4 * 128 * T].view(torch.int32).cpu().numpy().view(np.uint32).reshape(T, 128)
    np.testing.assert_array_equal(num, g[:, 1])
    for t in range(T):
        np.testing.assert_array_equal(lists[t, : num[t]], i[g[t, 0]: g[t, 0] + num[t]])
    fp.pack()
    assert_lists_equal(fp.lists_to_host(), g, i)
