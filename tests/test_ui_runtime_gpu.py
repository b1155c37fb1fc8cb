"""The RenderImGui node through the C++ host mirror: a `.renderer` text whose last two entries are the PostProcess Debug view into BackBuffer and RenderImGui,
as DefaultRenderer.renderer orders them, over test_tail_runtime_gpu's frame.  Draw data is handed over through the binding (Runtime.set_ui_draw_data) and drawn
by the node: BackBuffer equals the C-ABI sequence -- what the Debug view wrote, then sailor_hip_ui_draw over the flattened commands -- bit for bit.  Without
draw data, or with `color` unresolved, BackBuffer is what the Debug view wrote and nothing of ui_draw.hip is launched."""
import numpy as np
import pytest
import torch

import ui_cases as cases
import ui_ref as ref
from sailor_amd import host
from sailor_amd.forward_plus import UiPass
from sailor_amd.runtime_binding import load
from test_tail_runtime_gpu import DEBUG, DEBUG_VIEW, HEAD, Frame

pytestmark = pytest.mark.gpu

UI = """
- name: RenderImGui
  renderTargets:
  - color: %s
  - depthStencil: DepthBuffer
"""
UI_KERNELS = ["k_ui_scan", "k_ui_setup", "k_ui_blend"]


def text_of(color="BackBuffer"):
    return HEAD + DEBUG_VIEW % "#AO" + UI % color


def draw_data(W, H):
    """an editor-like frame: a translucent backdrop, a panel with an anti-aliased border, glyph quads under the panel's clip rect, callbacks between the draws, a
    second list with a clipped overlay"""
    a = cases.dl().clip(0, 0, W, H).rect(0, 0, W, H, host.ui_color(0.05, 0.05, 0.1, 0.35))
    a.clip(3.4, 2.6, W - 5.3, H - 3.2).rect_aa(5, 4, W - 8, H - 6, host.ui_color(0.2, 0.25, 0.3, 0.85), 1.0)
    a.callback(ref.CALLBACK_RESET)
    a.clip(6, 5, W - 9, H - 7)
    for k in range(40):
        x, y = 7 + 9 * (k % 10), 6 + 11 * (k // 10)
        a.quad(x, y, x + 8, y + 10, (0.25, 0.25), (0.75, 0.75), host.ui_color(1, 1, 0.9, 0.9))
    a.callback(ref.CALLBACK_USER)
    b = cases.dl().clip(W / 3, H / 4, W / 3, H / 2).rect(0, 0, W, H, cases.HALF_RED)   # an empty ClipRect: skipped
    b.clip(W / 2 + 0.7, H / 3, W + 40, H + 40).rect(W / 2 - 9, H / 3 - 5, W + 9, H - 3, cases.HALF_BLUE).rect(W / 2, H / 2, W - 2, H - 1, cases.HALF_GREEN)
    return host.ui_draw_data([a, b], (float(W), float(H)))


def frame_launches(fr):
    before, _ = fr.rt.launch_log(0)
    status = fr.process()
    after, names = fr.rt.launch_log(16)
    n = min(after - before, 16)
    return status, names[len(names) - n:] if n else []


def words(t):
    return t.cpu().numpy().view(np.uint32)


def test_the_node_is_registered():
    assert load().sailor_rt_node_registered(b"RenderImGui") == 1   # FrameGraph/RenderImGuiNode.cpp


def test_backbuffer_equals_the_c_abi_sequence_and_without_draw_data_it_is_the_debug_views(ctx):
    fr = Frame(text_of(), enable=(DEBUG,))
    try:
        assert fr.loaded[:2] == (6, 0)   # RenderImGui has a node class: created, not skipped
        W, H = fr.W, fr.H
        # no draw data: the Debug view's BackBuffer
        status, names = frame_launches(fr)
        assert status == 0 and names[-1] == "k_debug_view" and not [n for n in names if n.startswith("k_ui_")], (status, names)
        debug_view = fr.back.clone()
        assert not (debug_view == -3.0).all()
        # with draw data
        d = draw_data(W, H)
        flat = host.ui_flatten(d)
        assert (flat["width"], flat["height"]) == (W, H)
        assert fr.rt.set_ui_draw_data(d, font=cases.ATLAS) == len(flat["commands"]) == 4
        fr.back.fill_(-3.0)
        status, names = frame_launches(fr)
        assert status == 0 and names[-4:] == ["k_debug_view"] + UI_KERNELS, (status, names)
        up = UiPass(ctx, W, H)
        up.set_texture(cases.ATLAS)
        want = up.draw_flat(debug_view.clone(), flat, index_bytes=2)
        ctx.synchronize()
        np.testing.assert_array_equal(words(fr.back), words(want))
        assert (words(want) != words(debug_view)).any(axis=2).mean() > 0.9   # the backdrop touched the whole frame
        # ... which is the restatement's result as well
        s = dict(W=W, H=H, vertices=flat["vertices"], indices=flat["indices"], index_bytes=2, commands=flat["commands"], scale=flat["scale"], translate=flat["translate"],
                 texture=cases.ATLAS, target=debug_view.cpu().numpy())
        assert ref.same_bits_or_class(fr.back.cpu().numpy(), ref.render(s)["target"]).all()
        # a second frame draws the same data again; then the data is taken away
        fr.back.fill_(-3.0)
        status, names = frame_launches(fr)
        assert status == 0 and names[-3:] == UI_KERNELS
        np.testing.assert_array_equal(words(fr.back), words(want))
        assert fr.rt.set_ui_draw_data(None) == 0
        fr.back.fill_(-3.0)
        status, names = frame_launches(fr)
        assert status == 0 and names[-1] == "k_debug_view", names
        np.testing.assert_array_equal(words(fr.back), words(debug_view))
    finally:
        fr.close()


def test_with_color_unresolved_backbuffer_is_what_the_debug_view_wrote(ctx):
    fr = Frame(text_of("NoSuchTarget"), enable=(DEBUG,))
    try:
        assert fr.loaded[:2] == (6, 0)
        status, names = frame_launches(fr)
        debug_view = fr.back.clone()
        assert fr.rt.set_ui_draw_data(draw_data(fr.W, fr.H), font=cases.ATLAS) == 4
        fr.back.fill_(-3.0)
        status, names = frame_launches(fr)
        assert status == 0 and names[-1] == "k_debug_view" and not [n for n in names if n.startswith("k_ui_")], (status, names)
        np.testing.assert_array_equal(words(fr.back), words(debug_view))
    finally:
        fr.close()
