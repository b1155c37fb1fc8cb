"""GPU suite of the sky kernels through the C-ABI (sailor_hip_sky_fill, _sky_env_face, _sky_sun, _sky_compose, _sky_env_cubemap) against the fp32
restatement of tests/sky_ref.py.

Classification: a word is zero, finite or non-finite in exactly the places Ref32 says -- every branch of the kernels is geometry evaluated in Ref32's
order.  Values: every finite word within 1e-4 relative of Ref32, no texel outside (the 127-term sums of non-negative terms are the only thing the
kernel reassociates).  SUN and COMPOSE have no reassociated sum and are held bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import sky_cases as sc
import sky_ref as ref
from sailor_amd import _lib, host
from sailor_amd import forward_plus as fp

pytestmark = pytest.mark.gpu
f32 = np.float32
R32 = ref.Ref32()
REL = 1e-4
INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(ctx.device)


def held(got, want, what):
    """classification identical, finite values within REL, nobody outside; prints the figures before asserting"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == f32, (what, got.shape, want.shape)
    cg, cw = sc.classes(got), sc.classes(want)
    flips = int((cg != cw).sum())
    fin = cw == 1
    g, w = got[fin].astype(np.float64), want[fin].astype(np.float64)
    rel = np.abs(g - w) / np.abs(w) if fin.any() else np.zeros(1)
    outside = int((rel > REL).sum())
    print(f"{what}: {fin.sum()} finite non-zero words, class flips {flips}, max rel {rel.max():.3e}, outside {REL:g}: {outside}, "
          f"bit-equal {(bits(got) == bits(want)).mean():.4f}")
    assert flips == 0, f"{what}: {flips} words change class, first at {tuple(np.argwhere(cg != cw)[0])}"
    assert np.array_equal(bits(got)[cw != 1], bits(want)[cw != 1]), what
    assert outside == 0, f"{what}: {outside} words outside {REL:g} relative, max {rel.max():.3e}"


def same_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    bad = bits(got) != bits(want)
    assert got.shape == want.shape and not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {tuple(np.argwhere(bad)[0]) if bad.any() else None}"


@pytest.mark.parametrize("case", sc.CASES, ids=[c[0] for c in sc.CASES])
def test_fill_sun_compose_against_ref32(ctx, case):
    name, w, h, position, pitch, light, fov = case
    frame, params = sc.make_frame(w, h, position, pitch, fov), host.sky_params(lightDirection=light)
    U = sc.frame_uniforms(R32, frame, light)
    want_sky, want_sun = R32.fill(U, 48, 40), R32.sun(U, ref.SUN_RESOLUTION, ref.SUN_RESOLUTION)
    want = R32.compose(U, want_sky, want_sun, w, h)
    sky = fp.sky_fill(ctx, frame, params, 48, 40)
    sun = fp.sky_sun(ctx, frame, params, ref.SUN_RESOLUTION)
    out = fp.sky_compose(ctx, frame, params, dev(ctx, want_sky), dev(ctx, want_sun), w, h)
    chained = fp.sky_compose(ctx, frame, params, sky, sun, w, h)
    ctx.synchronize()
    assert np.any(want_sky[..., :3] > 0), "parity on a black sky shows nothing"
    held(sky, want_sky, f"{name} fill")
    same_bits(sun, want_sun, f"{name} sun")
    same_bits(out, want, f"{name} compose of Ref32's planes")
    held(chained, R32.compose(U, sky.cpu().numpy(), sun.cpu().numpy(), w, h), f"{name} compose of the kernels' planes")
    if name in sc.COMPOSE_SUN_INSIDE + sc.COMPOSE_SUN_OUTSIDE:
        assert sc.sun_window_changes(R32, U, want_sky, want, w, h) == (name in sc.COMPOSE_SUN_INSIDE), name


@pytest.mark.parametrize("env", sc.ENV_CASES, ids=[e[0] for e in sc.ENV_CASES])
def test_all_six_env_faces_against_ref32(ctx, env):
    name, position, light = env
    params, size = host.sky_params(lightDirection=light), 24
    chain = torch.zeros(fp.cube_chain_floats(size, 1), dtype=torch.float32, device=ctx.device)
    for face in range(6):
        fp.sky_env_face(ctx, position, params, chain, size, face)
    ctx.synchronize()
    got = chain.cpu().numpy().reshape(6, size, size, 4)
    lit = 0
    for face in range(6):
        want = R32.env_face(sc.face_uniforms(R32, face, position, light), size)
        held(got[face], want, f"{name} face {face}")
        lit += int(np.any(want > 1e-3))
    assert lit >= 4
    # the down face: rays through the Earth; whatever emerges behind it is scaled by the clamp of the canonical exp (2^-126), not by 0
    assert np.all(got[3][..., :3] < 1e-30)


def test_env_cubemap_is_six_faces_plus_the_mip_generator(ctx):
    params, position, size, levels = host.sky_params(), (0.0, 150.0, 0.0), 32, 6
    whole = fp.sky_env_cubemap(ctx, position, params, size, levels)
    parts = torch.zeros_like(whole)
    for face in range(6):
        fp.sky_env_face(ctx, position, params, parts, size, face)
    _lib.check(ctx._lib.sailor_hip_generate_mipmaps_cube(ctx.handle, parts.data_ptr(), size, levels), "sailor_hip_generate_mipmaps_cube", ctx.handle)
    ctx.synchronize()
    same_bits(whole, parts.cpu().numpy(), "sky_env_cubemap")
    offs, total = ref.chain_offsets(size, levels)
    assert total == whole.numel() and float(whole[offs[-1][0]:].abs().max()) > 0
    assert ctx.launches_of(lambda: fp.sky_env_cubemap(ctx, position, params, size, levels))[:6] == ["k_sky_march<env>"] * 6


def test_compose_over_two_bands_equals_the_whole_frame(ctx):
    c = sc.case("tele_sun")
    w, h, light = 80, 48, c.light
    frame, params = sc.make_frame(w, h, c.position, c.pitch, c.fov), host.sky_params(lightDirection=light)
    sky, sun = fp.sky_fill(ctx, frame, params, 32, 32), fp.sky_sun(ctx, frame, params, 16)
    whole = fp.sky_compose(ctx, frame, params, sky, sun, w, h)
    rows = []
    for rank in range(2):
        band = host.band_for_rank(w, h, rank, 2)
        rows.append((band.fbRowBegin, fp.sky_compose(ctx, frame, params, sky, sun, w, h, band=band)))
    ctx.synchronize()
    assert sum(r.shape[0] for _, r in rows) == h
    for begin, r in rows:
        same_bits(r, whole[begin:begin + r.shape[0]].cpu().numpy(), f"band at row {begin}")
    U = sc.frame_uniforms(R32, frame, light)
    b = host.band_for_rank(w, h, 1, 2)
    same_bits(rows[1][1], R32.compose(U, sky.cpu().numpy(), sun.cpu().numpy(), w, h, rows=(b.fbRowBegin, b.fbRowBegin + b.fbRowCount)), "Ref32 rows of band 1")


def test_argument_checks(ctx):
    lib, hnd = ctx._lib, ctx.handle
    frame, params = sc.make_frame(48, 32, (0.0, 150.0, 0.0), 0.0), host.sky_params()
    buf = torch.zeros(6 * 16 * 16 * 4, dtype=torch.float32, device=ctx.device)
    sky, sun, out = (torch.zeros((8, 8, 4), dtype=torch.float32, device=ctx.device) for _ in range(3))
    cam = (C.c_float * 3)(0.0, 150.0, 0.0)
    whole, bad_band = host.band_whole_frame(8, 8), _lib.Band(0, 1, 4, 8)
    F, P, p = C.byref(frame), C.byref(params), lambda t: t.data_ptr()
    refused = [
        lib.sailor_hip_sky_fill(None, F, P, p(buf), 16, 16), lib.sailor_hip_sky_fill(hnd, None, P, p(buf), 16, 16),
        lib.sailor_hip_sky_fill(hnd, F, None, p(buf), 16, 16), lib.sailor_hip_sky_fill(hnd, F, P, None, 16, 16),
        lib.sailor_hip_sky_fill(hnd, F, P, p(buf), 0, 16), lib.sailor_hip_sky_fill(hnd, F, P, p(buf), 16, 0), lib.sailor_hip_sky_fill(hnd, F, P, p(buf) + 4, 16, 16),
        lib.sailor_hip_sky_env_face(hnd, cam, P, p(buf), 16, 6), lib.sailor_hip_sky_env_face(hnd, cam, P, p(buf), 16, -1),
        lib.sailor_hip_sky_env_face(hnd, cam, P, p(buf), 0, 0), lib.sailor_hip_sky_env_face(hnd, None, P, p(buf), 16, 0),
        lib.sailor_hip_sky_env_face(hnd, cam, None, p(buf), 16, 0), lib.sailor_hip_sky_env_face(hnd, cam, P, None, 16, 0),
        lib.sailor_hip_sky_sun(hnd, F, P, None, 0, 0, None, 8, 8), lib.sailor_hip_sky_sun(hnd, F, P, None, 0, 0, p(sun), 0, 8),
        lib.sailor_hip_sky_sun(hnd, None, P, None, 0, 0, p(sun), 8, 8),
        lib.sailor_hip_sky_compose(hnd, F, P, None, 8, 8, p(sun), 8, 8, p(out), 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 8, 8, None, 8, 8, p(out), 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 8, 8, p(sun), 8, 8, None, 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 8, 8, p(sun), 8, 8, p(out), 8, 8, None),
        lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 8, 8, p(sun), 8, 8, p(out), 8, 8, C.byref(bad_band)),
        lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 8, 8, p(sun), 8, 8, p(sky), 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_compose(hnd, F, P, p(sky), 0, 8, p(sun), 8, 8, p(out), 8, 8, C.byref(whole)),
        lib.sailor_hip_sky_env_cubemap(hnd, cam, P, p(buf), 16, 0), lib.sailor_hip_sky_env_cubemap(hnd, cam, P, p(buf), 0, 1),
        lib.sailor_hip_sky_env_cubemap(hnd, cam, P, None, 16, 1),
    ]
    assert refused == [INVALID] * len(refused), refused
    assert lib.sailor_hip_sky_sun(hnd, F, P, p(sky), 8, 8, p(sun), 8, 8) == -7   # a clouds plane: unsupported until the cloud march exists
    ctx.synchronize()
    assert float(buf.abs().max()) == 0 and float(out.abs().max()) == 0   # a refused call records nothing


def test_launch_times_at_the_node_sizes(ctx):
    """prints the per-launch medians at SkyNode's sizes; asserts nothing about them (there is no parent to compare against)"""
    w, h = 3840, 2160
    frame, params = sc.make_frame(w, h, (0.0, 150.0, 0.0), 0.0), host.sky_params()
    chain = torch.zeros(fp.cube_chain_floats(256, 8), dtype=torch.float32, device=ctx.device)
    out = torch.empty((h, w, 4), dtype=torch.float32, device=ctx.device)
    sky, sun = fp.sky_fill(ctx, frame, params, 256), fp.sky_sun(ctx, frame, params, 32)
    times = {"fill 256x256": [], "sun 32x32": [], "compose 3840x2160": [], "env face 256x256": []}
    for it in range(12):
        ctx.time_launches(0, 4)
        fp.sky_fill(ctx, frame, params, 256)
        fp.sky_sun(ctx, frame, params, 32)
        fp.sky_compose(ctx, frame, params, sky, sun, w, h, out=out)
        fp.sky_env_face(ctx, (0.0, 150.0, 0.0), params, chain, 256, it % 6)
        ctx.synchronize()
        if it >= 2:
            for slot, key in enumerate(times):
                times[key].append(ctx.timed_launch_ms(slot))
    for key, v in times.items():
        print(f"sky launch {key}: median {np.median(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, n={len(v)})")
    assert all(len(v) == 10 and min(v) > 0 for v in times.values())
