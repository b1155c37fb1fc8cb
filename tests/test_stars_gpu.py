"""GPU suite of the star points and the sun-shaft pass through the C-ABI (sailor_hip_sky_stars, sailor_hip_sky_sun_shafts) against the fp32 restatement of
tests/stars_ref.py: every word BIT FOR BIT, non-finite words by class.  Nothing in these kernels is reassociated: the taps of the shafts accumulate in loop
order, and the stars of a pixel are added in index order."""
import ctypes as C

import numpy as np
import pytest
import torch

import sky_cases as skc
import stars_cases as sc
import stars_ref as sref
from sailor_amd import _lib, host
from sailor_amd import forward_plus as fp
from sailor_amd.forward_plus import HipContext, SkyStars

pytestmark = pytest.mark.gpu
f32 = np.float32
R32 = sref.Ref32()
INVALID = -1
FP = C.POINTER(C.c_float)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dev(ctx, a):
    return torch.from_numpy(np.array(a)).to(ctx.device)   # a copy: the shared references are read-only


def same_bits(got, want, what):
    """finite words bit for bit, non-finite words by class"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == f32, (what, got.shape, want.shape, got.dtype)
    cg, cw = skc.classes(got), skc.classes(want)
    assert np.array_equal(cg, cw), f"{what}: {int((cg != cw).sum())} words change class, first at {tuple(np.argwhere(cg != cw)[0])}"
    bad = (bits(got) != bits(want)) & (cw <= 1)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {at}: {got[at]!r} != {want[at]!r}, "
                             f"max abs {np.abs(got[bad].astype(np.float64) - want[bad]).max():.3e}")


def shafts_of(ctx, c, band=None, target=None):
    t = sc.shaft_target(c) if target is None else target
    b, n = (0, c.h) if band is None else (band.fbRowBegin, band.fbRowCount)
    return fp.sky_sun_shafts(ctx, sc.shaft_frame(c), sc.shaft_params(c), dev(ctx, sc.clouds_plane("ramp01", c.cw)), dev(ctx, t[b:b + n]), c.w, c.h, band=band)


def stars_of(ctx, c, band=None, clouds=True):
    frame, model, positions, colors, plane, target = sc.star_inputs(c.name)
    b, n = (0, c.h) if band is None else (band.fbRowBegin, band.fbRowCount)
    return SkyStars(ctx, positions, colors).draw(frame, model, dev(ctx, plane) if clouds else None, dev(ctx, target[b:b + n]), c.w, c.h, band=band)


@pytest.mark.parametrize("name", [c.name for c in sc.SHAFT_CASES])
def test_sun_shafts_against_ref32(ctx, name):
    c = sc.shaft_case(name)
    want, info, U = sc.shaft_reference(name)
    got = shafts_of(ctx, c)
    ctx.synchronize()
    g = got.cpu().numpy()
    print(f"{name}: uvView ({U['uvx']:.4g}, {U['uvy']:.4g}), early {U['early']}, taps clamped at the edges {info['edges']}; bit-equal words {(bits(g) == bits(want)).mean():.4f}")
    same_bits(g, want, name)
    assert np.isnan(want).any(), "the hostile texel"


def test_sun_shafts_with_a_nan_uv_view_walk_the_loop_inside_the_plane(ctx):
    """a NaN in projection makes uvView NaN: every comparison of the early-out fails, the loop runs with NaN coordinates from its second tap on, every tap is
    clamped into the plane and the result is NaN where Ref32's is"""
    c = sc.shaft_case("in_view_60")
    frame, params, plane, target = sc.shaft_frame(c), sc.shaft_params(c), sc.clouds_plane("ramp01", c.cw), sc.shaft_target(c)
    frame.projection[15] = float("nan")
    U = R32.shaft_uniforms(frame, params, c.cw, c.cw)
    want, _ = R32.sun_shafts(U, plane, target, c.w, c.h)
    got = fp.sky_sun_shafts(ctx, frame, params, dev(ctx, plane), dev(ctx, target), c.w, c.h)
    ctx.synchronize()
    assert np.isnan(U["uvx"]) and not U["early"] and np.isnan(want[..., 3]).all()
    same_bits(got, want, "NaN uvView")


@pytest.mark.parametrize("name", [c.name for c in sc.STAR_CASES])
def test_stars_against_ref32(ctx, name):
    c = sc.star_case(name)
    want, S = sc.star_reference(name)
    got = stars_of(ctx, c)
    ctx.synchronize()
    g = got.cpu().numpy()
    drawn = S["drop"] == 0
    print(f"{name}: {int(drawn.sum())} of {len(drawn)} stars drawn, {int((drawn & S['sky'] & (S['mask'] > 0)).sum())} lit, {int((drawn & ~S['sky']).sum())} on Earth-hitting rays, "
          f"at most {max(sc.stars_per_pixel(S, c.w).values(), default=0)} on a pixel; bit-equal words {(bits(g) == bits(want)).mean():.4f}")
    same_bits(g, want, name)
    if c.stars == "empty":
        assert np.array_equal(bits(g), bits(sc.star_inputs(name)[5]))


def test_stars_without_a_clouds_plane_see_the_cleared_one(ctx):
    c = sc.star_case("synthetic_96")
    want, _ = sc.run_stars(R32, c, clouds=False)
    got = stars_of(ctx, c, clouds=False)
    ctx.synchronize()
    same_bits(got, want, "NULL clouds")
    assert not np.array_equal(bits(want), bits(sc.star_reference(c.name)[0]))


@pytest.mark.parametrize("name", ["in_view_100", "fixture_131"])
def test_two_bands_equal_the_whole_target(ctx, name):
    shafts = name.startswith("in_view")
    c = sc.shaft_case(name) if shafts else sc.star_case(name)
    want = (sc.shaft_reference(name) if shafts else sc.star_reference(name))[0]
    for rank in range(2):
        band = host.band_for_rank(c.w, c.h, rank, 2)
        b, n = band.fbRowBegin, band.fbRowCount
        rows = shafts_of(ctx, c, band=band) if shafts else stars_of(ctx, c, band=band)
        ctx.synchronize()
        same_bits(rows, want[b:b + n], f"{name}: band at row {b}")
        ref_rows = sc.run_shafts(R32, c, rows=(b, b + n))[0] if shafts else sc.run_stars(R32, c, rows=(b, b + n))[0]
        same_bits(rows, ref_rows, f"{name}: Ref32 rows of the band at {b}")


def test_the_collision_case_gives_the_same_bits_on_every_run(ctx):
    c = sc.star_case("synthetic_96")
    runs = []
    for _ in range(2):
        runs.append(stars_of(ctx, c).clone())
        ctx.synchronize()
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    same_bits(runs[1], sc.star_reference(c.name)[0], "second run")


def test_captured_and_replayed_passes_equal_the_eager_ones(ctx):
    """stars, the clouds blit and the shafts, the three draws of "Stars & Clouds", captured on a side stream and replayed"""
    c = sc.star_case("synthetic_96")
    frame, model, positions, colors, plane, target0 = sc.star_inputs(c.name)
    params = sc.shaft_params(sc.shaft_case("in_view_60"))
    w, h = c.w, c.h
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        # every buffer the graph touches lives for the whole test and is filled before the side stream starts
        stars = SkyStars(c2, positions, colors)
        clouds, start, target = dev(c2, plane), dev(c2, target0), torch.empty((h, w, 4), dtype=torch.float32, device=ctx.device)
        lib, hnd, p = c2._lib, c2.handle, lambda t: t.data_ptr()
        band = host.band_whole_frame(w, h)
        m = np.ascontiguousarray(model, f32)
        assert lib.sailor_hip_sky_stars_bind_workspace(hnd, p(stars.workspace), stars.workspace.numel()) == 0

        def record():
            return [lib.sailor_hip_sky_stars(hnd, C.byref(frame), m.ctypes.data_as(FP), p(stars.positions), p(stars.colors), stars.count, p(clouds), c.cw, c.cw,
                                             p(target), w, h, C.byref(band)),
                    lib.sailor_hip_sky_blit_clouds(hnd, p(clouds), c.cw, c.cw, p(target), w, h, C.byref(band)),
                    lib.sailor_hip_sky_sun_shafts(hnd, C.byref(frame), C.byref(params), p(clouds), c.cw, c.cw, p(target), w, h, C.byref(band))]

        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            target.copy_(start)
        assert record() == [0] * 3   # once outside the capture, on the side stream
        torch.cuda.synchronize()
        eager = target.clone()
        want = R32.stars(frame, model, positions, colors, plane, target0, w, h)[0]
        import clouds_ref
        want = clouds_ref.Ref32().blit(plane, want, w, h)
        want = R32.sun_shafts(R32.shaft_uniforms(frame, params, c.cw, c.cw), plane, want, w, h)[0]
        same_bits(eager, want, "stars, blit, shafts")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            target.copy_(start)
            st = record()
        assert st == [0] * 3, st
        for _ in range(2):
            target.fill_(7.0)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(target.view(torch.int32), eager.view(torch.int32))
    finally:
        c2.close()


def test_argument_checks(ctx):
    lib, hnd = ctx._lib, ctx.handle
    c = sc.star_case("synthetic_96")
    frame, model, positions, colors, plane, _ = sc.star_inputs(c.name)
    params = sc.shaft_params(sc.shaft_case("in_view_60"))
    w, h = c.w, c.h
    stars = SkyStars(ctx, positions, colors)
    clouds = dev(ctx, plane)
    target = torch.full((h, w, 4), 3.0, dtype=torch.float32, device=ctx.device)
    big = torch.zeros((2 * h * w * 4,), dtype=torch.float32, device=ctx.device)   # a plane that holds the target's bytes inside
    whole, bad_band = host.band_whole_frame(w, h), _lib.Band(0, 1, 4, h)
    F, P, M, p = C.byref(frame), C.byref(params), np.ascontiguousarray(model, f32).ctypes.data_as(FP), lambda t: t.data_ptr()
    other = sc.star_frame(sc.star_case("fixture_131"))   # viewportSize (131, 77)
    zero, many, minus = sc.shaft_params(sc.shaft_case("in_view_60"), sunShaftsDistance=0), sc.shaft_params(sc.shaft_case("in_view_60"), sunShaftsDistance=1025), \
        sc.shaft_params(sc.shaft_case("in_view_60"), sunShaftsDistance=-3)

    def shafts(hd=hnd, f=F, q=P, cl=p(clouds), cw=c.cw, ch=c.cw, t=p(target), tw=w, th=h, b=C.byref(whole)):
        return lib.sailor_hip_sky_sun_shafts(hd, f, q, cl, cw, ch, t, tw, th, b)

    def draw(hd=hnd, f=F, m=M, ps=p(stars.positions), cs=p(stars.colors), n=stars.count, cl=p(clouds), cw=c.cw, ch=c.cw, t=p(target), tw=w, th=h, b=C.byref(whole)):
        return lib.sailor_hip_sky_stars(hd, f, m, ps, cs, n, cl, cw, ch, t, tw, th, b)

    assert lib.sailor_hip_sky_stars_bind_workspace(hnd, p(stars.workspace), stars.workspace.numel()) == 0
    refused = [
        shafts(hd=None), shafts(f=None), shafts(q=None), shafts(cl=None), shafts(t=None), shafts(b=None),
        shafts(cl=p(clouds) + 4), shafts(t=p(target) + 4), shafts(cw=0), shafts(ch=-1), shafts(tw=0), shafts(th=40000), shafts(b=C.byref(bad_band)),
        shafts(q=C.byref(zero)), shafts(q=C.byref(many)), shafts(q=C.byref(minus)),
        shafts(cl=p(target)), shafts(cl=p(target) + 16 * w), shafts(cl=p(big), cw=2 * w, ch=h, t=p(big) + 16 * w),
        draw(hd=None), draw(f=None), draw(m=None), draw(ps=None), draw(cs=None), draw(t=None), draw(b=None),
        draw(ps=p(stars.positions) + 4), draw(cs=p(stars.colors) + 4), draw(cl=p(clouds) + 4), draw(t=p(target) + 4), draw(cw=0), draw(tw=0), draw(b=C.byref(bad_band)),
        draw(n=-1), draw(n=65537), draw(f=C.byref(other)), draw(tw=131, th=77),
        draw(cl=p(target)), draw(cl=p(big), cw=2 * w, ch=h, t=p(big) + 16 * w), draw(ps=p(target)), draw(cs=p(target)),
        draw(t=p(stars.workspace)),
    ]
    assert refused == [INVALID] * len(refused), refused
    # no workspace, or too small a one
    assert lib.sailor_hip_sky_stars_bind_workspace(hnd, None, 0) == 0 and draw() == INVALID
    assert lib.sailor_hip_sky_stars_bind_workspace(hnd, p(stars.workspace), int(lib.sailor_hip_sky_stars_workspace_bytes(stars.count)) - 1) == 0 and draw() == INVALID
    assert lib.sailor_hip_sky_stars_bind_workspace(hnd, p(stars.workspace) + 4, 4096) == INVALID and lib.sailor_hip_sky_stars_bind_workspace(hnd, None, 16) == INVALID
    assert lib.sailor_hip_sky_stars_bind_workspace(None, p(stars.workspace), 4096) == INVALID
    assert b"workspace" in lib.sailor_hip_context_last_error(hnd)
    assert lib.sailor_hip_sky_stars_bind_workspace(hnd, p(stars.workspace), stars.workspace.numel()) == 0
    names = ctx.launches_of(lambda: (shafts(q=C.byref(many)), shafts(cl=p(target)), draw(n=65537), draw(f=C.byref(other)), draw(cl=p(target))))
    ctx.synchronize()
    assert names == [] and float((target - 3.0).abs().max()) == 0 and float(big.abs().max()) == 0   # a refused call records nothing
    # what is accepted: the ends of the distance range, count 0 without a mesh, a band without rows
    one, most = sc.shaft_params(sc.shaft_case("in_view_60"), sunShaftsDistance=1), sc.shaft_params(sc.shaft_case("in_view_60"), sunShaftsDistance=1024)
    assert ctx.launches_of(lambda: (shafts(q=C.byref(one)), shafts(q=C.byref(most)))) == ["k_sky_sun_shafts"] * 2
    assert ctx.launches_of(lambda: draw()) == ["k_sky_stars_project", "k_sky_stars_blend"]
    none = host.band_for_rank(w, h, 2, 8)   # four tile rows over eight ranks: this one has no rows
    assert none.fbRowCount == 0
    assert ctx.launches_of(lambda: (draw(n=0, ps=None, cs=None), draw(b=C.byref(none), t=None), shafts(b=C.byref(none), t=None))) == []
    assert draw(n=0, ps=None, cs=None) == 0 and draw(b=C.byref(none), t=None) == 0 and shafts(b=C.byref(none), t=None) == 0
    ctx.synchronize()


def test_launch_times_at_4k(ctx):
    """prints the per-launch medians at 3840 x 2160 with the shipped parameters (sunShaftsDistance 60, the catalogue's 9 110 stars, a 1080^2 clouds plane);
    asserts nothing about them (there is no parent to compare against)"""
    w, h, n = 3840, 2160, 1080
    c = sc.star_case("fixture_96")
    frame = skc.make_frame(w, h, c.position, c.pitch, c.fov)
    params = host.sky_params(lightDirection=(0.0, -0.1, 1.0))
    positions, colors, _ = sc.fixture_mesh()
    gen = torch.Generator(device=ctx.device).manual_seed(1)
    clouds = torch.rand((n, n, 4), dtype=torch.float32, device=ctx.device, generator=gen)
    target = torch.rand((h, w, 4), dtype=torch.float32, device=ctx.device, generator=gen)
    stars = SkyStars(ctx, positions, colors)
    model = host.sky_stars_model(list(frame.cameraPosition)[:3])
    times = {"stars project": [], "stars blend": [], "sun shafts": []}
    for it in range(7):
        ctx.time_launches(0, 3)
        stars.draw(frame, model, clouds, target, w, h)
        fp.sky_sun_shafts(ctx, frame, params, clouds, target, w, h)
        ctx.synchronize()
        if it >= 2:
            for slot, key in enumerate(times):
                times[key].append(ctx.timed_launch_ms(slot))
    for key, v in times.items():
        print(f"sky launch {key} 3840x2160: median {np.median(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, n={len(v)})")
    assert all(len(v) == 5 for v in times.values())
