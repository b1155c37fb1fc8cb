"""GPU suite of the clouds kernels through the C-ABI (sailor_hip_sky_clouds, _sky_sun_clouds, _sky_blit_clouds) against the fp32 restatement of
tests/clouds_ref.py: every word BIT FOR BIT, non-finite words by class.  Nothing in these kernels is reassociated: colorLow and transmittanceLow
accumulate in the shader's order and every exit is taken at the shader's step."""
import ctypes as C

import numpy as np
import pytest
import torch

import clouds_cases as cc
import clouds_ref as cref
import sky_cases as sc
import sky_ref
from sailor_amd import _lib, host
from sailor_amd import forward_plus as fp
from sailor_amd.forward_plus import HipContext

pytestmark = pytest.mark.gpu
f32 = np.float32
R32 = cref.Ref32()
INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dev(ctx, a):
    return torch.from_numpy(np.array(a)).to(ctx.device)   # a copy: the shared references are read-only


def same_bits(got, want, what):
    """finite words bit for bit, non-finite words by class"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == f32, (what, got.shape, want.shape, got.dtype)
    cg, cw = sc.classes(got), sc.classes(want)
    assert np.array_equal(cg, cw), f"{what}: {int((cg != cw).sum())} words change class, first at {tuple(np.argwhere(cg != cw)[0])}"
    bad = (bits(got) != bits(want)) & (cw <= 1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {at}: {got[at]!r} != {want[at]!r}, "
                             f"max abs {np.abs(got[bad].astype(np.float64) - want[bad]).max():.3e}")


def device_textures(ctx):
    return tuple(dev(ctx, t) for t in cc.textures())


def clouds_of(ctx, c, sky, tex, out=None, **overrides):
    frame = cc.make_frame(c)
    weather, low, high, noise = tex
    return fp.sky_clouds(ctx, frame, cc.params(c, **overrides), sky, weather, low, high, noise, dev(ctx, cc.depth_plane(c, frame)), c.w, c.h, out=out)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_clouds_plane_against_ref32(ctx, name):
    c = cc.case(name)
    sky, want, exit_step = cc.reference(name)
    lit, gone, early = cc.assert_coverage(c, want, exit_step)
    got = clouds_of(ctx, c, dev(ctx, sky), device_textures(ctx))
    ctx.synchronize()
    g = got.cpu().numpy()
    print(f"{name}: {lit} texels with alpha > 0, {gone} leave on transmittance, {early} return early; bit-equal words {(bits(g) == bits(want)).mean():.4f}")
    same_bits(g, want, name)


@pytest.mark.parametrize("time", [1.0e11, -3.0e10, 1.0e12, 3.0e38, float("inf"), float("nan")],
                         ids=["saturated_with_clouds", "saturated_negative", "all_saturated", "near_float_max", "inf", "nan"])
def test_hostile_texture_coordinates_stay_inside_the_planes(ctx, time):
    """currentTime drives the wind shifts (Sky.shader:394-397): at 1e11 the x and z taps of both volumes saturate at INT_MAX before they are wrapped while
    the y taps and the weather map do not, and the plane still has clouds; at -3e10 taps saturate at INT_MIN; at 1e12 every tap saturates; at 3e38 the
    shifts overflow to infinity; at inf the shift (0 * inf) * -0.2 is NaN.  No fetch may leave a plane, and every word equals Ref32's, whose conversion is
    the device's saturating one"""
    c = cc.case("under_up")
    frame, params = cc.make_frame(c), cc.params(c)
    frame.currentTime = time
    sky, _, _ = cc.reference(c.name)
    weather, low, high, noise = cc.textures()
    with np.errstate(all="ignore"):
        C = R32.context(sc.frame_uniforms(R32.G, frame, c.light), params, frame.currentTime, weather, low, high, noise)
        want, exit_step = R32.clouds(C, sky, cc.depth_plane(c, frame), frame.cameraZNearZFar[1], c.w, c.h)
    d = device_textures(ctx)
    got = fp.sky_clouds(ctx, frame, params, dev(ctx, sky), d[0], d[1], d[2], d[3], dev(ctx, cc.depth_plane(c, frame)), c.w, c.h)
    ctx.synchronize()
    print(f"currentTime {time}: alpha > 0 on {(want[..., 3] > 0).sum()} texels, non-finite words {(~np.isfinite(want)).sum()}, early {(exit_step == cref.EARLY).sum()}")
    same_bits(got, want, f"currentTime {time}")
    if time in (1.0e11, -3.0e10):
        assert (want[..., 3] > 0).sum() > 10, "the saturated taps show in no texel"


@pytest.mark.parametrize("w_kind", ["negative", "nan"])
def test_sun_behind_clouds_under_a_projection_with_a_negative_or_nan_w(ctx, w_kind):
    """uvView divides by its own w (Sky.shader:708).  A perspective projection keeps it in [0, 1]; a projection whose w row is scaled by 3 gives the sun
    behind the camera w = (3 z + 1) / 2 < 0 and finite mirrored coordinates; one with -inf in its corner makes projection * view, and with it w and the
    coordinates, NaN: NaN weights, a NaN alpha, `clouds < 0.5` false, every texel zero.  (w == 0 exactly needs a direction with view z == -1 exactly,
    which no texel of the sun plane has.)  Only this entry point reads frame.projection"""
    c = sc.case("level_sun_behind")
    frame, params = sc.make_frame(c.w, c.h, c.position, c.pitch, c.fov), host.sky_params(lightDirection=c.light)
    if w_kind == "negative":
        for k in (3, 7, 11):
            frame.projection[k] = 3.0 * frame.projection[k]
    else:
        frame.projection[15] = float("-inf")
    U = sc.frame_uniforms(R32.G, frame, c.light)
    plane = cc.alpha_plane("cells")
    with np.errstate(all="ignore"):
        want, (cu, cv, w) = R32.sun_clouds(U, cc.proj_view(frame), plane, sky_ref.SUN_RESOLUTION, sky_ref.SUN_RESOLUTION)
    got = fp.sky_sun_clouds(ctx, frame, params, dev(ctx, plane))
    ctx.synchronize()
    same_bits(got, want, w_kind)
    if w_kind == "negative":
        assert w.max() < 0 and np.isfinite(cu).all() and np.isfinite(cv).all() and (want[..., 0] > 0).any()
    else:
        assert np.isnan(w).all() and np.isnan(cu).all() and not want.any()


@pytest.mark.parametrize("kind", ["ramp", "cells"])
@pytest.mark.parametrize("name", ["tele_sun", "wide_low_sun", "level_sun_behind"])
def test_sun_behind_clouds_against_ref32(ctx, name, kind):
    c = sc.case(name)
    frame, params = sc.make_frame(c.w, c.h, c.position, c.pitch, c.fov), host.sky_params(lightDirection=c.light)
    U = sc.frame_uniforms(R32.G, frame, c.light)
    plane = cc.alpha_plane(kind)
    want, (cu, cv, w) = R32.sun_clouds(U, cc.proj_view(frame), plane, sky_ref.SUN_RESOLUTION, sky_ref.SUN_RESOLUTION)
    plain = R32.G.sun(U, sky_ref.SUN_RESOLUTION, sky_ref.SUN_RESOLUTION)
    got = fp.sky_sun_clouds(ctx, frame, params, dev(ctx, plane))
    ctx.synchronize()
    same_bits(got, want, f"{name} {kind}")
    hidden = int(((plain[..., 0] > 0) & (want[..., 0] == 0)).sum())
    shown = int((want[..., 0] > 0).sum())
    print(f"{name} {kind}: {shown} sun texels shown, {hidden} hidden; w in [{w.min():.3g}, {w.max():.3g}]")
    if name == "level_sun_behind":   # the sun behind the camera: uvView's w is small and positive, the coordinates lie far outside [0, 1] and are clamped to the edge
        assert 0 < w.min() and w.max() < 0.1 and cu.min() > 1 and cv.min() > 1
    elif name == "tele_sun":         # the sun dead centre of the lens: the alpha plane straddles 0.5 across its footprint
        assert w.min() > 0.99 and shown > 100 and hidden > 100, (shown, hidden)


def test_sun_behind_a_clear_plane_is_the_plain_sun(ctx):
    c = sc.case("tele_sun")
    frame, params = sc.make_frame(c.w, c.h, c.position, c.pitch, c.fov), host.sky_params(lightDirection=c.light)
    got = fp.sky_sun_clouds(ctx, frame, params, dev(ctx, cc.alpha_plane("zero")))
    plain = fp.sky_sun(ctx, frame, params)
    ctx.synchronize()
    assert float(plain.max()) > 0
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    # a NaN alpha hides the sun: `clouds < 0.5` is false
    nan_plane = cc.alpha_plane("zero")
    nan_plane[..., 3] = np.nan
    got = fp.sky_sun_clouds(ctx, frame, params, dev(ctx, nan_plane))
    ctx.synchronize()
    assert float(got.abs().max()) == 0


def blit_inputs():
    rng = np.random.default_rng(cc.SEED + 2)
    w, h = 80, 48
    clouds = cc.alpha_plane("ramp", 24, 16)
    clouds[..., :3] = rng.random((16, 24, 3)).astype(f32) * 20.0
    clouds[3, 5] = (np.inf, -np.inf, np.nan, 0.25)
    target = (rng.random((h, w, 4)).astype(f32) * 10.0 - 2.0).astype(f32)
    return w, h, clouds, target


def test_blit_against_ref32_and_two_bands_equal_the_whole_frame(ctx):
    w, h, clouds, target = blit_inputs()
    want = R32.blit(clouds, target, w, h)
    d_clouds = dev(ctx, clouds)
    whole = fp.sky_blit_clouds(ctx, d_clouds, dev(ctx, target), w, h)
    ctx.synchronize()
    same_bits(whole, want, "blit")
    assert np.isnan(want).any() and np.isinf(want).any()
    for rank in range(2):
        band = host.band_for_rank(w, h, rank, 2)
        b, n = band.fbRowBegin, band.fbRowCount
        rows = fp.sky_blit_clouds(ctx, d_clouds, dev(ctx, target[b:b + n]), w, h, band=band)
        ctx.synchronize()
        same_bits(rows, want[b:b + n], f"band at row {b}")
        same_bits(rows, R32.blit(clouds, target[b:b + n], w, h, rows=(b, b + n)), f"Ref32 rows of band at {b}")


def chain(ctx, c, tex, sky_size, target):
    """the four launches of the node with clouds: Clouds, Sun, Compose, Blit Clouds (SkyNode.cpp:565-731)"""
    frame, params = cc.make_frame(c), cc.params(c)
    w, h = 2 * c.w, 2 * c.h
    weather, low, high, noise = tex
    sky = fp.sky_fill(ctx, frame, params, sky_size)
    clouds = fp.sky_clouds(ctx, frame, params, sky, weather, low, high, noise, dev(ctx, cc.depth_plane(c, frame)), c.w, c.h)
    sun = fp.sky_sun_clouds(ctx, frame, params, clouds, 16)
    fp.sky_compose(ctx, frame, params, sky, sun, w, h, out=target)
    return fp.sky_blit_clouds(ctx, clouds, target, w, h)


def test_captured_and_replayed_chain_equals_the_eager_one(ctx):
    c = cc.case("under_up")
    w, h = 2 * c.w, 2 * c.h
    eager = chain(ctx, c, device_textures(ctx), 16, torch.zeros((h, w, 4), dtype=torch.float32, device=ctx.device)).clone()
    ctx.synchronize()
    assert float(eager[..., 3].abs().max()) > 0, "the blit left no alpha: no clouds in the chain"
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        # every buffer the graph touches lives for the whole test and is filled before the side stream starts: a tensor freed while a kernel of another
        # stream still uses it would be handed to the next allocation
        tex = device_textures(c2)
        target = torch.full((h, w, 4), 7.0, dtype=torch.float32, device=ctx.device)
        depth = dev(c2, cc.depth_plane(c, cc.make_frame(c)))
        frame, params = cc.make_frame(c), cc.params(c)
        weather, low, high, noise = tex
        sky = torch.empty((16, 16, 4), dtype=torch.float32, device=ctx.device)
        clouds = torch.empty((c.h, c.w, 4), dtype=torch.float32, device=ctx.device)
        sun = torch.empty((16, 16, 4), dtype=torch.float32, device=ctx.device)
        lib, hnd, F, P, p = c2._lib, c2.handle, C.byref(frame), C.byref(params), lambda t: t.data_ptr()
        band = host.band_whole_frame(w, h)

        def record():
            return [lib.sailor_hip_sky_fill(hnd, F, P, p(sky), 16, 16),
                    lib.sailor_hip_sky_clouds(hnd, F, P, p(sky), 16, 16, p(weather), 32, 32, p(low), 16, p(high), 8, p(noise), 16, 16, p(depth), w, h, p(clouds), c.w, c.h),
                    lib.sailor_hip_sky_sun_clouds(hnd, F, P, p(clouds), c.w, c.h, p(sun), 16, 16),
                    lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 16, 16, p(sun), 16, 16, p(target), w, h, C.byref(band)),
                    lib.sailor_hip_sky_blit_clouds(hnd, p(clouds), c.w, c.h, p(target), w, h, C.byref(band))]

        torch.cuda.synchronize()
        assert record() == [0] * 5   # once outside the capture, on the side stream
        torch.cuda.synchronize()
        assert torch.equal(target.view(torch.int32), eager.view(torch.int32))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st = record()
        assert st == [0] * 5, st
        for _ in range(2):
            target.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(target.view(torch.int32), eager.view(torch.int32))
    finally:
        c2.close()


def test_argument_checks(ctx):
    lib, hnd = ctx._lib, ctx.handle
    c = cc.case("under_up")
    frame, params = cc.make_frame(c), cc.params(c)
    weather, low, high, noise = device_textures(ctx)
    sky, out, target = (torch.zeros((8, 8, 4), dtype=torch.float32, device=ctx.device) for _ in range(3))
    depth = torch.zeros((8, 8), dtype=torch.float32, device=ctx.device)
    whole, bad_band = host.band_whole_frame(8, 8), _lib.Band(0, 1, 4, 8)
    F, P, p = C.byref(frame), C.byref(params), lambda t: t.data_ptr()

    def clouds(h=hnd, f=F, q=P, s=p(sky), sw=8, m=p(weather), mw=32, l=p(low), ln=16, g=p(high), gn=8, n=p(noise), nw=16, d=p(depth), dw=8, o=p(out), ow=8):
        return lib.sailor_hip_sky_clouds(h, f, q, s, sw, 8, m, mw, 32, l, ln, g, gn, n, nw, 16, d, dw, 8, o, ow, 8)

    eleven, minus = cc.params(c), cc.params(c)
    eleven.scatteringSteps, minus.scatteringSteps = 11, -1
    refused = [
        clouds(h=None), clouds(f=None), clouds(q=None), clouds(s=None), clouds(m=None), clouds(l=None), clouds(g=None), clouds(n=None), clouds(d=None), clouds(o=None),
        clouds(s=p(sky) + 4), clouds(m=p(weather) + 4), clouds(l=p(low) + 1), clouds(g=p(high) + 1), clouds(n=p(noise) + 4), clouds(d=p(depth) + 4), clouds(o=p(out) + 4),
        clouds(sw=0), clouds(mw=0), clouds(ln=0), clouds(gn=-1), clouds(nw=0), clouds(dw=0), clouds(ow=0),
        clouds(o=p(sky)), clouds(q=C.byref(eleven)), clouds(q=C.byref(minus)),
        lib.sailor_hip_sky_sun_clouds(None, F, P, p(sky), 8, 8, p(out), 8, 8), lib.sailor_hip_sky_sun_clouds(hnd, None, P, p(sky), 8, 8, p(out), 8, 8),
        lib.sailor_hip_sky_sun_clouds(hnd, F, None, p(sky), 8, 8, p(out), 8, 8), lib.sailor_hip_sky_sun_clouds(hnd, F, P, None, 8, 8, p(out), 8, 8),
        lib.sailor_hip_sky_sun_clouds(hnd, F, P, p(sky), 8, 8, None, 8, 8), lib.sailor_hip_sky_sun_clouds(hnd, F, P, p(sky) + 4, 8, 8, p(out), 8, 8),
        lib.sailor_hip_sky_sun_clouds(hnd, F, P, p(sky), 0, 8, p(out), 8, 8), lib.sailor_hip_sky_sun_clouds(hnd, F, P, p(sky), 8, 8, p(out), 8, 0),
        lib.sailor_hip_sky_sun_clouds(hnd, F, P, p(out), 8, 8, p(out), 8, 8),
        lib.sailor_hip_sky_blit_clouds(None, p(sky), 8, 8, p(target), 8, 8, C.byref(whole)), lib.sailor_hip_sky_blit_clouds(hnd, None, 8, 8, p(target), 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_blit_clouds(hnd, p(sky), 8, 8, None, 8, 8, C.byref(whole)), lib.sailor_hip_sky_blit_clouds(hnd, p(sky), 8, 8, p(target), 8, 8, None),
        lib.sailor_hip_sky_blit_clouds(hnd, p(sky), 8, 8, p(target), 8, 8, C.byref(bad_band)), lib.sailor_hip_sky_blit_clouds(hnd, p(sky), 8, 8, p(target) + 4, 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_blit_clouds(hnd, p(sky), 8, 0, p(target), 8, 8, C.byref(whole)), lib.sailor_hip_sky_blit_clouds(hnd, p(sky), 8, 8, p(target), 0, 8, C.byref(whole)),
        lib.sailor_hip_sky_blit_clouds(hnd, p(target), 8, 8, p(target), 8, 8, C.byref(whole)),
    ]
    assert refused == [INVALID] * len(refused), refused
    names = ctx.launches_of(lambda: (clouds(q=C.byref(eleven)), clouds(o=p(sky)), lib.sailor_hip_sky_blit_clouds(hnd, p(target), 8, 8, p(target), 8, 8, C.byref(whole))))
    ctx.synchronize()
    assert names == [] and float(out.abs().max()) == 0 and float(target.abs().max()) == 0 and float(sky.abs().max()) == 0   # a refused call records nothing
    ten = cc.params(c)
    ten.scatteringSteps = 10
    assert clouds(q=C.byref(ten)) == 0 and ctx.launches_of(lambda: clouds()) == ["k_sky_clouds"]
    ctx.synchronize()
