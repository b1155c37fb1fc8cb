"""The RenderImGui pass (sailor_amd/csrc/ui_draw.hip) through the C-ABI against tests/ui_ref.py: the target bit for bit on all four channels (a non-finite
value by class) -- every case and every soup of tests/ui_cases.py on the whole frame, in every band of a two-way and a three-way split, with 16-bit and with
32-bit indices, and under hipGraph capture with two replays onto a restored target; the golden file; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import ui_cases as cases
import ui_ref as ref
from make_ui_golden import PATH as GOLDEN, golden_scene
from sailor_amd import _lib, host
from sailor_amd.forward_plus import HipContext, UiPass

pytestmark = pytest.mark.gpu


def dev(ctx, a, view=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view is not None else a).to(ctx.device)


class Uploaded:
    """a scene's buffers on the device"""

    def __init__(self, ctx, s, index_bytes=None):
        self.index_bytes = index_bytes or s["index_bytes"]
        self.vertices = dev(ctx, s["vertices"].view(np.uint8)) if len(s["vertices"]) else torch.zeros(20, dtype=torch.uint8, device=ctx.device)
        idx = np.asarray(s["indices"], np.uint32)
        if self.index_bytes == 2:
            assert len(idx) == 0 or idx.max() < 65536
            idx = idx.astype(np.uint16).view(np.int16)
        else:
            idx = idx.view(np.int32)
        self.indices = dev(ctx, idx) if len(idx) else torch.zeros(4, dtype=torch.int16 if self.index_bytes == 2 else torch.int32, device=ctx.device)
        self.num_indices = len(idx)
        self.commands = np.ascontiguousarray(s["commands"], _lib.UI_COMMAND_DTYPE)
        self.d_commands = dev(ctx, self.commands.view(np.uint8)) if len(self.commands) else None
        self.target = dev(ctx, np.zeros((s["H"], s["W"], 4), np.float32) if s.get("target") is None else s["target"])


def make_pass(ctx, s, band=None):
    up = UiPass(ctx, s["W"], s["H"], band, max_triangles=ref.num_triangles(s))
    up.set_texture(s.get("texture"))
    return up


def record(up, u, s, target):
    return up.draw(target, u.vertices, u.indices, u.commands, u.d_commands, s["scale"], s["translate"])


def run(ctx, s, band=None, u=None, index_bytes=None):
    """the scene through sailor_hip_ui_draw -> the band's rows of the target"""
    u = u or Uploaded(ctx, s, index_bytes)
    up = make_pass(ctx, s, band)
    r0, r1 = up.band.fbRowBegin, up.band.fbRowBegin + up.band.fbRowCount
    target = u.target[r0:r1].clone()
    record(up, u, s, target)
    ctx.synchronize()
    return target.cpu().numpy()


def assert_same(got, want, what=""):
    same = ref.same_bits_or_class(got, want)
    assert same.all(), f"{what}: {(~same).sum()} words of the target differ, first at {np.argwhere(~same)[:4].tolist()}"


SCENES = list(cases.CASES) + [f"soup_{seed}" for seed in range(cases.NUM_SOUPS)]


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: ref.render(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


@pytest.mark.parametrize("name", SCENES)
def test_every_case_and_soup_against_the_restatement_whole_banded_and_in_both_index_widths(ctx, scenes, rendered, name):
    s = scenes[name]
    want = rendered[name]["target"]
    for index_bytes in (2, 4):
        u = Uploaded(ctx, s, index_bytes)
        assert_same(run(ctx, s, u=u), want, f"{name}, {8 * index_bytes}-bit indices")
        if index_bytes != s["index_bytes"]:
            continue
        for world in (2, 3):   # a band's result is the band's rows of the whole frame's (tests/test_ui_cpu.py holds the restatement to that)
            seen = 0
            for rank in range(world):
                band = host.band_for_rank(s["W"], s["H"], rank, world)
                r0, r1 = band.fbRowBegin, band.fbRowBegin + band.fbRowCount
                assert_same(run(ctx, s, band=band, u=u), want[r0:r1], f"{name} band {rank}/{world}")
                seen += r1 - r0
            assert seen == s["H"]


def test_under_graph_capture_and_two_replays_onto_a_restored_target(ctx, scenes, rendered):
    names = ("chunk_seam_513", "glyphs", "soup_3")
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        us = [Uploaded(c2, scenes[n]) for n in names]
        ups = [make_pass(c2, scenes[n]) for n in names]
        work = [u.target.clone() for u in us]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for n, u, up, t in zip(names, us, ups, work):
                t.copy_(u.target)   # the pass blends in place: every replay starts from the seed
                record(up, u, scenes[n], t)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for n, t in zip(names, work):
                assert_same(t.cpu().numpy(), rendered[n]["target"], f"{n} replayed")
    finally:
        c2.close()


def test_golden_file(ctx):
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        assert_same(run(ctx, golden_scene(g, name)), g[f"{name}.target"], name)


def test_nothing_to_draw_launches_nothing_and_a_bin_no_record_touches_stores_nothing(ctx, scenes):
    s = scenes["zero_commands"]
    u, up = Uploaded(ctx, s), make_pass(ctx, s)
    target = u.target.clone()
    assert ctx.launches_of(lambda: record(up, u, s, target)) == []
    s = scenes["scissor_zero_extent"]   # commands and triangles, but every box is empty
    u, up = Uploaded(ctx, s), make_pass(ctx, s)
    target = u.target.clone()
    assert ctx.launches_of(lambda: record(up, u, s, target)) == ["k_ui_scan", "k_ui_setup", "k_ui_blend"]
    ctx.synchronize()
    assert torch.equal(target.view(torch.int32), u.target.view(torch.int32))
    # an empty band (a frame of one tile row split in two) records nothing
    s = scenes["shared_diagonal"]
    empty = [b for b in (host.band_for_rank(72, 16, r, 2) for r in range(2)) if b.fbRowCount == 0]
    assert len(empty) == 1
    u = Uploaded(ctx, s)
    up = UiPass(ctx, 72, 16, empty[0], max_triangles=2)
    none = torch.zeros((0, 72, 4), dtype=torch.float32, device=ctx.device)
    lib = ctx._lib
    scale, translate = (C.c_float * 2)(0.1, 0.1), (C.c_float * 2)(-1, -1)
    tex = _lib.TextureDesc(None, 0, 0, 0, 0)
    short = u.commands.copy()
    short["scissor"][0] = [0, 0, 72, 16]   # (the scissor is checked against the frame, whatever the band)
    call = lambda: lib.sailor_hip_ui_draw(ctx.handle, u.vertices.data_ptr(), 4, u.indices.data_ptr(), 2, 6, short.ctypes.data, u.d_commands.data_ptr(), 1, scale,  # noqa: E731
                                          translate, C.byref(tex), up.workspace.data_ptr(), up.workspace.numel(), none.data_ptr() or None, 72, 16, C.byref(empty[0]))
    st = []
    assert ctx.launches_of(lambda: st.append(call())) == [] and st == [0], (st, lib.sailor_hip_context_last_error(ctx.handle).decode())


def test_refusals(ctx, scenes):
    s = scenes["shared_diagonal"]
    W, H = s["W"], s["H"]
    u, up = Uploaded(ctx, s), make_pass(ctx, s)
    lib, hnd = ctx._lib, ctx.handle
    target = u.target.clone()
    scale, translate = (C.c_float * 2)(*s["scale"]), (C.c_float * 2)(*s["translate"])
    tex = up._texture
    ws, n = up.workspace.data_ptr(), up.workspace.numel()
    needed = C.c_size_t()
    assert lib.sailor_hip_ui_workspace_bytes(2, W, H, C.byref(needed)) == 0

    def cmds(**kw):
        c = u.commands.copy()
        for k, v in kw.items():
            c[k][0] = v
        return c

    def draw(v=u.vertices.data_ptr(), nv=4, i=u.indices.data_ptr(), ib=2, ni=6, c=u.commands, dc=u.d_commands.data_ptr(), nc=1, sc=scale, tr=translate, tx=tex, w=ws,
             nb=n, t=target.data_ptr(), width=W, height=H, band=up.band):
        keep = np.ascontiguousarray(c)
        return lib.sailor_hip_ui_draw(hnd, v, nv, i, ib, ni, keep.ctypes.data if c is not None else None, dc, nc, sc, tr, C.byref(tx) if tx is not None else None, w, nb,
                                      t, width, height, C.byref(band) if band is not None else None)

    def refused(call, text):
        st = []
        launched = ctx.launches_of(lambda: st.append(call()))
        assert st[0] == -1 and launched == [], (st, launched, text)
        assert text in lib.sailor_hip_context_last_error(hnd).decode(), lib.sailor_hip_context_last_error(hnd).decode()

    refused(lambda: draw(v=None), "vertex buffer")
    refused(lambda: draw(v=u.vertices.data_ptr() + 2), "vertex buffer")
    refused(lambda: draw(i=None), "index buffer")
    refused(lambda: draw(i=u.indices.data_ptr() + 2, ib=4), "index buffer")
    refused(lambda: draw(i=u.indices.data_ptr() + 1), "index buffer")
    refused(lambda: draw(ib=3), "index width")
    refused(lambda: draw(ib=8), "index width")
    refused(lambda: draw(c=None), "command array")
    refused(lambda: draw(dc=None), "command array")
    refused(lambda: draw(dc=u.d_commands.data_ptr() + 2), "command array")
    refused(lambda: draw(nc=_lib.UI_MAX_COMMANDS + 1), "SAILOR_UI_MAX_COMMANDS")
    refused(lambda: draw(sc=None), "scale, translate or the texture")
    refused(lambda: draw(tr=None), "scale, translate or the texture")
    refused(lambda: draw(tx=None), "scale, translate or the texture")
    refused(lambda: draw(tx=_lib.TextureDesc(tex.texels, tex.width, tex.height, _lib.TEXTURE_SRGB, 0)), "sRGB")
    refused(lambda: draw(tx=_lib.TextureDesc(tex.texels + 2, tex.width, tex.height, 0, 0)), "texels")
    refused(lambda: draw(t=None), "the target")
    refused(lambda: draw(t=target.data_ptr() + 4), "the target")
    refused(lambda: draw(w=None), "the workspace is NULL")
    refused(lambda: draw(w=ws + 4), "the workspace is NULL or not 16-byte aligned")
    refused(lambda: draw(nb=needed.value - 1), "smaller than")
    refused(lambda: draw(width=0), "extent")
    refused(lambda: draw(height=-3), "extent")
    refused(lambda: draw(band=None), "band")
    refused(lambda: draw(band=_lib.Band(0, 1, 3, 16)), "band")
    refused(lambda: draw(ni=5), "index range")
    refused(lambda: draw(c=cmds(firstIndex=1)), "index range")
    refused(lambda: draw(c=cmds(firstIndex=0xFFFFFFFF)), "index range")
    for bad in ([-1, 0, 10, 10], [0, -1, 10, 10], [0, 0, -1, 10], [0, 0, 10, -1], [W - 5, 0, 6, 10], [0, H - 5, 10, 6], [0x7FFFFFFF, 0, 0x7FFFFFFF, 1]):
        refused(lambda: draw(c=cmds(scissor=bad)), "scissor")
    ctx.synchronize()
    assert torch.equal(target.view(torch.int32), u.target.view(torch.int32))
    assert draw(nb=needed.value) == 0   # exactly the size query's answer is enough
    ctx.synchronize()
    assert_same(target.cpu().numpy(), ref.render(s)["target"], "after the refusals")
