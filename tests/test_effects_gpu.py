"""GPU suite of the post-effect kernels through the C-ABI (sailor_hip_blur, sailor_hip_chromatic_aberration, sailor_hip_blit_linear) against the fp32
restatement of tests/effects_ref.py, BIT FOR BIT: the images are compared as uint32 words; only the radius-1e30 case compares a NaN by class.  Every
case of tests/effects_cases.py, the kernel each call launches, every refusal, the committed golden, and one print-only timing at 4K."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import effects_cases as ec
import effects_ref as ref
import make_effects_golden as golden
from effects_ref import Ref32
from sailor_amd import _lib, host
from sailor_amd.forward_plus import Blur, ChromaticAberration, blit_linear

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
KERNEL = dict(gauss="k_blur_gauss", radial="k_blur_radial", aberration="k_chromatic_aberration", blit="k_blit_linear")


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(ctx.device)


def same_words(got: torch.Tensor, want: np.ndarray, what: str, nan_by_class=False):
    g = np.ascontiguousarray(got.cpu().numpy(), f32)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    ok = g.view(np.uint32) == np.ascontiguousarray(want, f32).view(np.uint32)
    if nan_by_class:
        ok |= np.isnan(g) & np.isnan(want)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} words differ from the restatement, first at {tuple(np.argwhere(~ok)[0])}"


def record(ctx, c, src):
    """records case c's one call on the device tensor `src`; returns the output it fills (-7 beforehand)"""
    if c.kind in ("gauss", "radial"):
        p = Blur(ctx, c.width, c.height, c.defines, host.blur_params(**c.params))
    elif c.kind == "aberration":
        p = ChromaticAberration(ctx, c.width, c.height, host.chromatic_aberration_params(**c.params))
    else:
        out = torch.full((c.height, c.width) + c.src.shape[2:], -7.0, dtype=torch.float32, device=ctx.device)
        return blit_linear(ctx, src, out)
    p.out.fill_(-7.0)
    return p.run(src)


@pytest.mark.parametrize("name", list(ec.cases()))
def test_case_bit_for_bit(ctx, name):
    c = ec.cases()[name]
    want = ec.run(Ref32, c)
    src = dev(ctx, c.src)
    out = []
    assert ctx.launches_of(lambda: out.append(record(ctx, c, src))) == [KERNEL[c.kind]]
    ctx.synchronize()
    same_words(out[0], want, name, nan_by_class=c.by_class)


def test_refusals_return_minus_one_leave_the_output_and_record_nothing(ctx):
    c = ec.cases()["gauss_HORIZONTAL_128x96"]
    lib, hnd, p = ctx._lib, ctx.handle, lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    W, H = c.width, c.height
    big = torch.full((2 * H, W, 4), -7.0, dtype=torch.float32, device=ctx.device)   # the output and, for the overlap cases, the source share it
    out, src = big[:H], dev(ctx, c.src)
    count = C.c_uint64()
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    before = count.value
    nan, inf = float("nan"), float("inf")
    G = lambda **kw: C.byref(host.blur_params(**dict(dict(blurRadius=4.0), **kw)))
    R = lambda **kw: C.byref(host.blur_params(**dict(ref.RADIAL_SHIPPED, **kw)))
    A = lambda *offset: C.byref(host.chromatic_aberration_params(offset=offset))
    blur, aberration, blit = lib.sailor_hip_blur, lib.sailor_hip_chromatic_aberration, lib.sailor_hip_blit_linear
    ok_gauss = (hnd, p(src), W, H, G(), _lib.BLUR_HORIZONTAL, p(out), W, H)
    ok_radial = (hnd, p(src), W, H, R(), _lib.BLUR_RADIAL, p(out), W, H)
    ok_aberration = (hnd, p(src), W, H, A(0.1, 0.2, 0.3), p(out), W, H)
    ok_blit = (hnd, p(src), W, H, p(out), W // 2, H // 2, 4)

    def refused(fn, args, index, value):
        a = list(args)
        a[index] = value
        assert fn(*a) == -1, (fn.__name__, index, value)

    too_big = 32769
    # (function, a valid call, the indices of: the pointers and params, the planes, the extents)
    for fn, ok, nulls, planes, extents in ((blur, ok_gauss, (0, 1, 4, 6), (1, 6), (2, 3, 7, 8)), (blur, ok_radial, (0, 1, 4, 6), (1, 6), (2, 3, 7, 8)),
                                           (aberration, ok_aberration, (0, 1, 4, 5), (1, 5), (2, 3, 6, 7)), (blit, ok_blit, (0, 1, 4), (1, 4), (2, 3, 5, 6))):
        for i in nulls:
            refused(fn, ok, i, None)
        for i in planes:                                  # not 16-byte aligned
            refused(fn, ok, i, p(big, 16 * W * H + 4)), refused(fn, ok, i, p(big, 16 * W * H + 8))
        for i in extents:                                 # outside extent_ok
            refused(fn, ok, i, 0), refused(fn, ok, i, -3), refused(fn, ok, i, too_big)
        refused(fn, ok, planes[0], p(out))                # the output is the source
        last_row = 16 * (W // 2) * (H // 2 - 1) if fn is blit else 16 * W * (H - 1)
        refused(fn, ok, planes[0], p(big, last_row))      # ... or begins in its last row
    for flags in (8, 16, 1 << 31, 0xFFFFFFF8 | _lib.BLUR_HORIZONTAL):   # unknown flag bits
        refused(blur, ok_gauss, 5, flags)
    for r in (nan, inf, -inf, -1.0, -1e-30, 4294967296.0, 1e30):        # Gauss: uint() of these is undefined
        refused(blur, ok_gauss, 4, G(blurRadius=r))
    for r in (nan, inf, -inf):                                         # radial: the radius and the centre must be finite
        refused(blur, ok_radial, 4, R(blurRadius=r)), refused(blur, ok_radial, 4, R(blurCenter=(r, 0.5))), refused(blur, ok_radial, 4, R(blurCenter=(0.5, r)))
    for n in (nan, inf, -inf, 0.0, 0.99, -4.0, 256.5, 1e9):            # ... and the count finite, within [1, 256]
        refused(blur, ok_radial, 4, R(blurSampleCount=n))
    for bad in (nan, inf, -inf):                                       # aberration: offset.xyz finite
        refused(aberration, ok_aberration, 4, A(bad, 0.0, 0.0)), refused(aberration, ok_aberration, 4, A(0.0, bad, 0.0)), refused(aberration, ok_aberration, 4, A(0.0, 0.0, bad))
    for channels in (0, 2, 3, 5, -1, 16):
        refused(blit, ok_blit, 7, channels)
    refused(blit, (hnd, p(src), W, H, p(out, 4), W // 2, H // 2, 4), 0, hnd)   # four channels need 16-byte alignment (4 suffices for one: below)
    refused(blit, (hnd, p(src), W, H, p(out, 2), W // 2, H // 2, 1), 0, hnd)   # one channel needs 4-byte alignment
    ctx.synchronize()
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    assert count.value == before, "a refused call recorded a launch"
    assert (big[:H] == -7.0).all(), "a refused call wrote the output"

    # what is legal: an adjacent, non-overlapping source; radius >= 12 and the largest radius below 2^32; a 4-byte aligned one-channel plane; alpha of
    # the parameters that the shader does not read may be anything
    adjacent = big[H:]
    adjacent.copy_(src)
    accepted = [
        blur(hnd, p(adjacent), W, H, G(), _lib.BLUR_HORIZONTAL, p(out), W, H),
        blur(hnd, p(adjacent), W, H, G(blurRadius=4294967040.0), 0, p(out), W, H),
        blur(hnd, p(adjacent), W, H, R(blurSampleCount=(256.0, nan, nan, nan), blurRadius=(20.0, inf, nan, -1.0)), _lib.BLUR_RADIAL, p(out), W, H),
        aberration(hnd, p(adjacent), W, H, C.byref(host.chromatic_aberration_params(offset=(0.1, 0.2, 0.3, nan))), p(out), W, H),
        blit(hnd, p(adjacent), W, H, p(out), W // 2, H // 2, 4),
        blit(hnd, p(adjacent, 4), W, H, p(out, 4), W // 2, H // 2, 1),
    ]
    ctx.synchronize()
    assert accepted == [0] * 6, accepted
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    assert count.value == before + 6


def test_golden(ctx):
    g = np.load(ROOT / "tests" / "golden" / "tiny_effects.npz")
    (w, h), (bw, bh) = (int(x) for x in g["target"]), (int(x) for x in g["blit_target"])
    color, plane = g["color_bits"].view(f32), g["plane_bits"].view(f32)
    radius, count, cx, cy = (float(x) for x in g["radial_params"])
    d_color, d_plane = dev(ctx, color), dev(ctx, plane)
    empty = lambda *shape: torch.empty(shape, dtype=torch.float32, device=ctx.device)
    got = dict(
        gauss=Blur(ctx, w, h, "HORIZONTAL", host.blur_params(blurRadius=float(g["gauss_radius"][0]))).run(d_color),
        radial=Blur(ctx, w, h, "RADIAL", host.blur_params(blurRadius=radius, blurSampleCount=count, blurCenter=(cx, cy))).run(d_color),
        aberration=ChromaticAberration(ctx, w, h, host.chromatic_aberration_params(offset=g["offset"])).run(d_color),
        blit4=blit_linear(ctx, d_color, empty(bh, bw, 4)), blit1=blit_linear(ctx, d_plane, empty(bh, bw)))
    ctx.synchronize()
    for name, out in got.items():
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), g[name + "_bits"], err_msg=name)
    # the golden is the restatement's: it has not drifted
    assert (w, h) == (golden.W, golden.H) and (bw, bh) == golden.BLIT
    for name, want in golden.outputs(color, plane).items():
        np.testing.assert_array_equal(want.view(np.uint32), g[name + "_bits"], err_msg=name)


def test_launch_times_at_4k(ctx):
    """prints the per-launch medians at 3840 x 2160; asserts nothing about them (there is no parent to compare against)"""
    w, h = 3840, 2160
    gen = torch.Generator(device=ctx.device).manual_seed(1)
    color = torch.rand((h, w, 4), dtype=torch.float32, device=ctx.device, generator=gen)
    quarter = torch.empty((512, 512, 4), dtype=torch.float32, device=ctx.device)
    passes = {"gauss H radius 4": Blur(ctx, w, h, "HORIZONTAL", host.blur_params(blurRadius=4.0)), "gauss H radius 12": Blur(ctx, w, h, "HORIZONTAL", host.blur_params(blurRadius=12.0)),
              "radial 20 / 10": Blur(ctx, w, h, "RADIAL"), "aberration": ChromaticAberration(ctx, w, h)}
    times = {k: [] for k in list(passes) + ["blit 3840x2160 -> 512x512"]}
    for it in range(7):
        ctx.time_launches(0, 5)
        for p in passes.values():
            p.run(color)
        blit_linear(ctx, color, quarter)
        ctx.synchronize()
        if it >= 2:
            for slot, key in enumerate(times):
                times[key].append(ctx.timed_launch_ms(slot))
    for key, v in times.items():
        print(f"effects launch {key} 3840x2160: median {np.median(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, n={len(v)})")
    assert all(len(v) == 5 for v in times.values())
