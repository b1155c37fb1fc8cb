"""GPU suite of the tail kernels through the C-ABI (sailor_hip_motion_blur, sailor_hip_debug_view) against the fp32 restatement of tests/tail_ref.py,
BIT FOR BIT: the images are compared as uint32 words; where a hostile depth makes a NaN, the word is compared by class (its payload is the hardware's).
Every case of tests/tail_cases.py, the kernels each call launches, every refusal, the committed golden, and one print-only timing at 4K."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import tail_cases as tc
import tail_ref as ref
from sailor_amd import _lib, host
from sailor_amd.forward_plus import DebugView, MotionBlur
from tail_ref import Ref32

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
MODES = {"": ref.SCENE, "AO": ref.AO, "LIGHT_TILES": ref.LIGHT_TILES, "CASCADES": ref.CASCADES}


def dev(ctx, a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(ctx.device)


def same_words(got: torch.Tensor, want: np.ndarray, what: str, nan_by_class=False):
    g = np.ascontiguousarray(got.cpu().numpy(), f32)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    ok = g.view(np.uint32) == np.ascontiguousarray(want, f32).view(np.uint32)
    if nan_by_class:
        ok |= np.isnan(g) & np.isnan(want)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} words differ from the restatement, first at {tuple(np.argwhere(~ok)[0])}"


def run_blur(ctx, c):
    mb = MotionBlur(ctx, c.width, c.height, host.motion_blur_params(**c.params))
    mb.out.fill_(-7.0)
    out = mb.run(c.frame, c.previous, dev(ctx, c.depth), dev(ctx, c.color))
    ctx.synchronize()
    return out


@pytest.mark.parametrize("name", list(tc.blur_cases()))
def test_motion_blur_case_bit_for_bit(ctx, name):
    c = tc.blur_cases()[name]
    want = Ref32.motion_blur(c.frame, c.previous, c.depth, c.color, c.params, c.width, c.height)
    same_words(run_blur(ctx, c), want, name, nan_by_class=name.startswith("hostile"))


@pytest.mark.parametrize("size", list(tc.debug_cases()))
@pytest.mark.parametrize("define", list(MODES))
def test_debug_view_mode_bit_for_bit(ctx, size, define):
    c = tc.debug_cases()[size]
    want = Ref32.debug_view(c.frame, MODES[define], c.width, c.height, **tc.debug_args(c, MODES[define]))
    dv = DebugView(ctx, c.width, c.height, define)
    dv.out.fill_(-7.0)
    out = dv.run(c.frame, dev(ctx, c.scene), dev(ctx, c.linear_depth), dev(ctx, c.grid, np.uint32), dev(ctx, c.culled, np.uint32), dev(ctx, c.ao))
    ctx.synchronize()
    same_words(out, want, f"{size} {define or 'SCENE'}")


def test_debug_view_ignores_what_its_mode_does_not_read(ctx):
    """the lists are ignored outside LIGHT_TILES, the scene outside SCENE / CASCADES: None for them is accepted"""
    c = tc.debug_cases()["131x77"]
    for define, args in (("", dict(scene=c.scene)), ("AO", dict(ao=c.ao)), ("CASCADES", dict(scene=c.scene, linear_depth=c.linear_depth)),
                         ("LIGHT_TILES", dict(linear_depth=c.linear_depth, lights_grid=c.grid, culled_lights=c.culled))):
        ints = ("lights_grid", "culled_lights")
        out = DebugView(ctx, c.width, c.height, define).run(c.frame, **{k: dev(ctx, v, np.uint32 if k in ints else f32) for k, v in args.items()})
        ctx.synchronize()
        same_words(out, Ref32.debug_view(c.frame, MODES[define], c.width, c.height, **tc.debug_args(c, MODES[define])), define)


def test_each_call_launches_exactly_its_kernel(ctx):
    c, d = tc.blur_cases()["yaw_128x96"], tc.debug_cases()["128x96"]
    mb = MotionBlur(ctx, c.width, c.height)
    depth, color = dev(ctx, c.depth), dev(ctx, c.color)
    assert ctx.launches_of(lambda: mb.run(c.frame, c.previous, depth, color)) == ["k_motion_blur"]
    t = [dev(ctx, d.scene), dev(ctx, d.linear_depth), dev(ctx, d.grid, np.uint32), dev(ctx, d.culled, np.uint32), dev(ctx, d.ao)]
    for define in MODES:
        dv = DebugView(ctx, d.width, d.height, define)
        assert ctx.launches_of(lambda: dv.run(d.frame, *t)) == ["k_debug_view"], define
    ctx.synchronize()


def test_refusals_return_minus_one_leave_the_output_and_record_nothing(ctx):
    c, d = tc.blur_cases()["yaw_128x96"], tc.debug_cases()["128x96"]
    lib, hnd, p = ctx._lib, ctx.handle, lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    W, H = c.width, c.height
    depth, color = dev(ctx, c.depth), dev(ctx, c.color)
    big = torch.full((2 * H, W, 4), -7.0, dtype=torch.float32, device=ctx.device)   # the output and, for the overlap case, the colour share it
    out = big[:H]
    scene, linear, ao = dev(ctx, d.scene), dev(ctx, d.linear_depth), dev(ctx, d.ao)
    grid, culled = dev(ctx, d.grid, np.uint32), dev(ctx, d.culled, np.uint32)
    fr, pv = C.byref(c.frame), C.byref(c.previous)
    P = lambda **kw: C.byref(host.motion_blur_params(**kw))
    count = C.c_uint64()
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    before = count.value
    blur = lib.sailor_hip_motion_blur
    ok = (hnd, fr, pv, p(depth), W, H, p(color), W, H, P(), p(out), W, H)

    def refused(index, value, fn=blur, args=ok):
        a = list(args)
        a[index] = value
        assert fn(*a) == -1, (index, value)

    for i in (0, 1, 2, 3, 6, 9, 10):        # null context, frame, previous frame, depth, colour, params, output
        refused(i, None)
    refused(3, p(depth, 2)), refused(6, p(color, 4)), refused(10, p(out, 8))     # misaligned
    for i in (4, 5, 7, 8, 11, 12):          # non-positive extents
        refused(i, 0), refused(i, -3)
    for s in (float("nan"), float("inf"), 0.5, 0.0, -2.0, 64.5, 1e9):
        refused(9, P(samples=s))
    refused(9, P(maxSpeed=0.0)), refused(9, P(maxSpeed=-0.0))
    refused(6, p(out)), refused(6, p(big, 16 * W * (H - 1)))                    # the output is, or overlaps, the colour
    assert blur(hnd, fr, pv, p(depth), W, H, p(big, 16 * W * H), W, H, P(), p(out), W, H) == 0   # adjacent is not overlapping
    ctx.synchronize()
    out.fill_(-7.0)
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    assert count.value == before + 1
    before = count.value

    view = lib.sailor_hip_debug_view
    sw, sh, aw, ah = d.scene.shape[1], d.scene.shape[0], d.ao.shape[1], d.ao.shape[0]
    okv = [hnd, C.byref(d.frame), 0, p(scene), sw, sh, p(linear), W, H, p(grid), p(culled), p(ao), aw, ah, p(out), W, H]
    mode = lambda m: okv[:2] + [m] + okv[3:]
    for m in (-1, 4, 99):
        refused(2, m, view, okv)
    for m in range(4):
        refused(0, None, view, mode(m)), refused(1, None, view, mode(m)), refused(14, None, view, mode(m)), refused(14, p(out, 4), view, mode(m))
        refused(15, 0, view, mode(m)), refused(16, -1, view, mode(m))
    for m in (ref.SCENE, ref.CASCADES):     # a mode that needs a buffer it was given as null
        refused(3, None, view, mode(m)), refused(3, p(scene, 4), view, mode(m)), refused(4, 0, view, mode(m)), refused(3, p(out), view, mode(m))
    for m in (ref.LIGHT_TILES, ref.CASCADES):
        refused(6, None, view, mode(m)), refused(7, 0, view, mode(m))
    refused(9, None, view, mode(ref.LIGHT_TILES)), refused(10, None, view, mode(ref.LIGHT_TILES))
    refused(15, W - 16, view, mode(ref.LIGHT_TILES)), refused(16, H + 16, view, mode(ref.LIGHT_TILES))   # the target is not the frame
    refused(11, None, view, mode(ref.AO)), refused(12, 0, view, mode(ref.AO))
    ctx.synchronize()
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    assert count.value == before, "a refused call recorded a launch"
    assert (big[:H] == -7.0).all(), "a refused call wrote the output"


def test_golden(ctx):
    g = np.load(ROOT / "tests" / "golden" / "tiny_tail.npz")
    h, w = g["depth_bits"].shape
    frame, previous = _lib.UboFrameData.from_buffer_copy(g["frame"].tobytes()), _lib.UboFrameData.from_buffer_copy(g["previous"].tobytes())
    intensity, samples, max_speed = (float(x) for x in g["params"])
    mb = MotionBlur(ctx, w, h, host.motion_blur_params(intensity=intensity, samples=samples, maxSpeed=max_speed))
    out = mb.run(frame, previous, dev(ctx, g["depth_bits"].view(f32)), dev(ctx, g["color_bits"].view(f32)))
    ctx.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), g["blur_bits"])
    dv = DebugView(ctx, w, h, "LIGHT_TILES")
    out = dv.run(frame, None, dev(ctx, g["linear_bits"].view(f32)), dev(ctx, g["grid"], np.uint32), dev(ctx, g["culled"], np.uint32))
    ctx.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), g["tiles_bits"])
    # the golden is the restatement's: it has not drifted
    want = Ref32.motion_blur(frame, previous, g["depth_bits"].view(f32), g["color_bits"].view(f32), dict(intensity=intensity, samples=samples, maxSpeed=max_speed), w, h)
    np.testing.assert_array_equal(want.view(np.uint32), g["blur_bits"])


def test_launch_times_at_4k(ctx):
    """prints the per-launch medians at 3840 x 2160 with the shipped parameters; asserts nothing about them (there is no parent to compare against)"""
    w, h = 3840, 2160
    cam, prev = tc.camera(w, h), tc.camera(w, h, yaw=0.05)
    gen = torch.Generator(device=ctx.device).manual_seed(1)
    color = torch.rand((h, w, 4), dtype=torch.float32, device=ctx.device, generator=gen)
    depth = torch.rand((h, w), dtype=torch.float32, device=ctx.device, generator=gen) * 0.1 + 1e-3
    linear = 1.0 / depth
    tx, ty = tc.tiles_of(w, h)
    grid = torch.zeros((tx * ty, 2), dtype=torch.int32, device=ctx.device)
    grid[:, 0] = 1 + torch.arange(tx * ty, device=ctx.device, dtype=torch.int32) * 128
    grid[:, 1] = 32
    culled = torch.zeros(tx * ty * 128 + 1, dtype=torch.int32, device=ctx.device)
    mb = MotionBlur(ctx, w, h)
    views = {d: DebugView(ctx, w, h, d) for d in MODES}
    times = {"motion blur": [], "debug scene": [], "debug AO": [], "debug LIGHT_TILES": [], "debug CASCADES": []}
    for it in range(7):
        ctx.time_launches(0, 5)
        mb.run(cam.frame, prev.frame, depth, color)
        for d in MODES:
            views[d].run(cam.frame, color, linear, grid, culled, linear)
        ctx.synchronize()
        if it >= 2:
            for slot, key in enumerate(times):
                times[key].append(ctx.timed_launch_ms(slot))
    for key, v in times.items():
        print(f"tail launch {key} 3840x2160: median {np.median(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, n={len(v)})")
    assert all(len(v) == 5 for v in times.values())
