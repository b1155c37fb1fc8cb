"""The DebugDraw pass (sailor_amd/csrc/debug_lines.hip) through the C-ABI against tests/lines_ref.py: keys, Main and DepthBuffer bit for bit (a NaN colour by
class) -- every case and every soup of tests/lines_cases.py on the whole frame and in every band of a two-way split, with and without an index buffer, once
under hipGraph capture; the golden file; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import lines_cases as cases
import lines_ref as ref
from make_lines_golden import PATH as GOLDEN, golden_scene
from sailor_amd import _lib, host
from sailor_amd.forward_plus import DebugLinesPass, HipContext

pytestmark = pytest.mark.gpu


def dev(ctx, a, view=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view is not None else a).to(ctx.device)


class Uploaded:
    """a scene's buffers on the device"""

    def __init__(self, ctx, s):
        self.vertices = dev(ctx, s["vertices"].view(np.uint8))
        self.indices = None if s.get("indices") is None else dev(ctx, s["indices"], np.int32)
        self.depth = dev(ctx, np.zeros((s["H"], s["W"]), np.float32) if s.get("depth") is None else s["depth"])
        self.target = dev(ctx, np.zeros((s["H"], s["W"], 4), np.float32) if s.get("target") is None else s["target"])


def run(ctx, s, band=None, up=None, dp=None):
    """the scene through begin / draw / resolve -> dict like lines_ref.render's"""
    up = up or Uploaded(ctx, s)
    dp = dp or DebugLinesPass(ctx, s["W"], s["H"], band)
    r0, r1 = dp.band.fbRowBegin, dp.band.fbRowBegin + dp.band.fbRowCount
    depth, target = up.depth.clone(), up.target[r0:r1].clone()
    dp.begin(depth)
    dp.draw(s["vp"], up.vertices, up.indices, ref.num_segments(s), s.get("prim_base", 0))
    dp.resolve(target, depth)
    return dict(keys=dp.download_keys(), target=target.cpu().numpy(), depth=depth.cpu().numpy())


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got["keys"], want["keys"], err_msg=f"{what}: keys")
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), err_msg=f"{what}: depth")
    same = ref.same_bits_or_class(got["target"], want["target"])
    assert same.all(), f"{what}: {(~same).sum()} words of Main differ, first at {np.argwhere(~same)[:4].tolist()}"


SCENES = list(cases.CASES) + [f"soup_{seed}" for seed in range(cases.NUM_SOUPS)]


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: ref.render(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


@pytest.mark.parametrize("name", SCENES)
def test_every_case_and_soup_against_the_restatement_whole_and_banded(ctx, scenes, rendered, name):
    s = scenes[name]
    up = Uploaded(ctx, s)
    assert_same(run(ctx, s, up=up), rendered[name], name)
    bands = 0
    for rank in range(2):   # bands are whole tile rows: a frame of one tile row has one band, the whole frame
        band = host.band_for_rank(s["W"], s["H"], rank, 2)
        if band.fbRowCount == 0 or band.fbRowCount == s["H"]:
            continue
        assert_same(run(ctx, s, band=band, up=up), ref.render(s, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)), f"{name} band {rank}/2")
        bands += 1
    assert bands == (2 if s["H"] > 16 else 0)


def test_an_identity_index_buffer_changes_nothing(ctx, scenes, rendered):
    for name in ("octant_star", "through_each_side_plane", "hand_over_65", "soup_2"):
        s = dict(scenes[name])
        assert s.get("indices") is None
        s["indices"] = np.arange(len(s["vertices"]), dtype=np.uint32)
        assert_same(run(ctx, s), rendered[name], f"{name} with the identity index buffer")


def test_under_graph_capture(ctx, scenes, rendered):
    names = ("hand_over_tall", "soup_6")
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        ups = [Uploaded(c2, scenes[n]) for n in names]
        dps = [DebugLinesPass(c2, scenes[n]["W"], scenes[n]["H"]) for n in names]
        work = [(u.depth.clone(), u.target.clone()) for u in ups]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for n, u, dp, (d, t) in zip(names, ups, dps, work):
                d.copy_(u.depth); t.copy_(u.target)   # the pass rewrites both in place: every replay starts from the seeds
                dp.begin(d)
                dp.draw(scenes[n]["vp"], u.vertices, u.indices, ref.num_segments(scenes[n]), scenes[n].get("prim_base", 0))
                dp.resolve(t, d)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for n, dp, (d, t) in zip(names, dps, work):
                assert_same(dict(keys=dp.download_keys(), target=t.cpu().numpy(), depth=d.cpu().numpy()), rendered[n], f"{n} replayed")
    finally:
        c2.close()


def test_golden_file(ctx):
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        got = run(ctx, golden_scene(g, name))
        np.testing.assert_array_equal(got["keys"], g[f"{name}.keys"])
        assert ref.same_bits_or_class(got["target"], g[f"{name}.target"]).all()
        np.testing.assert_array_equal(got["depth"].view(np.uint32), g[f"{name}.depth_out"].view(np.uint32))


def test_a_frame_with_no_segments_launches_nothing(ctx, scenes):
    s = scenes["horizontal"]
    up, dp = Uploaded(ctx, s), DebugLinesPass(ctx, s["W"], s["H"])
    depth, target = up.depth.clone(), up.target.clone()
    dp.begin(depth)

    def nothing():
        dp.draw(s["vp"], up.vertices, None, 0)
        dp.resolve(target, depth)
    assert ctx.launches_of(nothing) == []
    assert torch.equal(target, up.target) and torch.equal(depth, up.depth)


def test_refusals(ctx, scenes):
    s = scenes["horizontal"]
    W, H = s["W"], s["H"]
    up, dp = Uploaded(ctx, s), DebugLinesPass(ctx, W, H)
    lib, hnd = ctx._lib, ctx.handle
    ws, n = dp.workspace.data_ptr(), dp.workspace.numel()
    vp = (C.c_float * 16)(*[float(x) for x in s["vp"]])
    depth, target = up.depth.clone(), up.target.clone()
    dp.begin(depth)
    ctx.synchronize()
    keys = dp.download_keys().copy()
    good = _lib.DebugLinesDraw(up.vertices.data_ptr(), None, 2, 0)
    bad_band = _lib.Band(0, 1, 3, 16)

    def refused(call, text):
        launched = []
        st = []
        launched += ctx.launches_of(lambda: st.append(call()))
        assert st[0] == -1 and launched == [], (st, launched)
        assert text in lib.sailor_hip_context_last_error(hnd).decode(), lib.sailor_hip_context_last_error(hnd).decode()

    draw = lambda d=good, band=dp.band, w=ws, nb=n, m=vp: lib.sailor_hip_debug_lines_draw(hnd, m, C.byref(d) if d is not None else None, W, H, C.byref(band), w, nb)  # noqa: E731
    res = lambda d=good, t=target.data_ptr(), z=depth.data_ptr(): lib.sailor_hip_debug_lines_resolve(hnd, vp, C.byref(d), W, H, C.byref(dp.band), ws, n, t, z)  # noqa: E731
    refused(lambda: draw(d=None), "the matrix or the draw is NULL")
    refused(lambda: draw(m=None), "the matrix or the draw is NULL")
    refused(lambda: draw(band=bad_band), "the band is not valid")
    refused(lambda: draw(w=ws + 4), "16-byte aligned")
    refused(lambda: draw(nb=64), "too small")
    refused(lambda: draw(d=_lib.DebugLinesDraw(None, None, 2, 0)), "vertex buffer")
    refused(lambda: draw(d=_lib.DebugLinesDraw(up.vertices.data_ptr(), up.vertices.data_ptr() + 2, 2, 0)), "index buffer")
    refused(lambda: draw(d=_lib.DebugLinesDraw(up.vertices.data_ptr(), None, 2, 0xFFFFFFFD)), "reaches 2^32 - 1")
    refused(lambda: res(t=None), "the target is NULL")
    refused(lambda: res(t=target.data_ptr() + 4), "the target is NULL or not 16-byte aligned")
    refused(lambda: res(z=None), "the depth attachment")
    refused(lambda: res(d=_lib.DebugLinesDraw(up.vertices.data_ptr(), None, 2, 0xFFFFFFFD)), "reaches 2^32 - 1")
    ctx.synchronize()
    np.testing.assert_array_equal(dp.download_keys(), keys)
    assert torch.equal(target, up.target) and torch.equal(depth, up.depth)
    assert lib.sailor_hip_debug_lines_draw(hnd, vp, C.byref(_lib.DebugLinesDraw(up.vertices.data_ptr(), None, 2, 0xFFFFFFFC)), W, H, C.byref(dp.band), ws, n) == 0
