"""Inputs shared by the clouds tests: seeded synthetic textures, cameras, and helpers that run a restatement of tests/clouds_ref.py on a case.

Textures: a 32 x 32 RGBA8 weather map, a 16^3 and an 8^3 R8 volume -- white noise smoothed with wrap-around and stretched to the full byte range, so that
clouds are patchy --, and the 16 x 16 noise of the HBAO tests (tests/golden/hbao_noise.npy, decoded as the HBAO path decodes it).

Cameras cover the three origin branches of CloudsMarching (Sky.shader:468-494): under the layer (cameraPosition.y = 150 cm), inside it (1.5e6 cm) and above
it, looking down.  The camera above stands at 1e7 cm, not 3e6, because every case has to contain rays that return early, and from above only :500 can do that
(:463 needs cloudsEndIntersections.x < 0, which from outside the outer sphere means a miss, and then both shifts are 0).  From 30 km the tangent to the
layer's inner sphere is 541 km long: no first hit lies beyond BigDistance = 600 km.  From 40 km the band of such rays is 0.02 degrees wide; from 100 km
it is 1.8 degrees (tangent 1 088 km), about one row of a 16-row plane with a 40 degree lens.  An inside camera returns early only behind the wall.

A case also fixes currentTime, scatteringSteps and the linearDepth plane: "far" = zFar everywhere, "wall" = a near wall (5 000 units) on the left half.
With scatteringSteps = 0 the loop of :547 never runs: transmittanceLow stays 1, alpha 0, and no ray can leave on transmittance -- that case is required
to have dense steps and early returns only (see coverage()).
"""
import functools
from collections import namedtuple

import numpy as np

import clouds_ref as cref
import sky_cases as sc
import sky_ref
from hbao_cases import noise_texels
from sailor_amd import host

f32 = np.float32
SEED = 20240611
SKY = 16   # the sky plane the CLOUDS draw samples (the node: 256)
WALL = 5000.0

Case = namedtuple("Case", "name w h position pitch light fov time steps depth")
CASES = [
    Case("under_up", 24, 16, (0.0, 150.0, 0.0), 20.0, sc.SUN_HIGH, 90.0, 0.0, 5, "far"),
    Case("under_wall_time", 72, 10, (300.0, 150.0, -200.0), 25.0, sc.SUN_LOW_UP, 90.0, 12.5, 2, "wall"),
    Case("inside_level", 72, 10, (0.0, 1.5e6, 0.0), 0.0, sc.SUN_DEFAULT, 90.0, 3.0, 5, "wall"),
    Case("inside_wall_one_octave", 24, 16, (5.0e5, 1.5e6, 2.0e5), -10.0, sc.SUN_HIGH, 90.0, 0.0, 1, "wall"),
    Case("above_down", 24, 16, (0.0, 1.0e7, 0.0), -25.0, sc.SUN_HIGH, 40.0, 0.0, 5, "far"),
    Case("above_down_no_scattering", 24, 16, (0.0, 1.0e7, 0.0), -20.0, sc.SUN_DEFAULT, 40.0, 7.0, 0, "far"),
    Case("under_two_octaves_low_sun", 24, 16, (0.0, 150.0, 0.0), 12.0, sc.SUN_LOW_AHEAD, 90.0, 1.0, 2, "far"),
]


def case(name):
    return next(c for c in CASES if c.name == name)


def _smooth(rng, shape, passes):
    a = rng.random(shape)
    for _ in range(passes):
        for ax in range(a.ndim):
            a = (np.roll(a, 1, ax) + a + np.roll(a, -1, ax)) / 3.0
    a = (a - a.min()) / (a.max() - a.min())
    return a


@functools.lru_cache(maxsize=None)
def textures():
    """(weather uint8 (32, 32, 4), low uint8 (16, 16, 16), high uint8 (8, 8, 8), noise float32 (16, 16, 4))"""
    rng = np.random.default_rng(SEED)
    weather = np.stack([_smooth(rng, (32, 32), 2) for _ in range(4)], -1)
    weather[..., 2] = 0.35 + 0.65 * weather[..., 2]   # b: the height the cloud tops reach
    weather[..., 3] = 0.5 + 0.5 * weather[..., 3]     # a: density
    to8 = lambda a: np.ascontiguousarray(np.round(a * 255.0).astype(np.uint8))
    low = to8(_smooth(rng, (16, 16, 16), 1) ** 0.5)
    high = to8(_smooth(rng, (8, 8, 8), 1))
    return to8(weather), low, high, np.ascontiguousarray(noise_texels(), f32)


def make_frame(c):
    """sky_cases' camera with the case's currentTime"""
    frame = sc.make_frame(c.w, c.h, c.position, c.pitch, c.fov)
    frame.currentTime = c.time
    return frame


def params(c, **overrides):
    return host.sky_params(lightDirection=c.light, scatteringSteps=c.steps, **overrides)


def depth_plane(c, frame, w=None, h=None):
    """linearDepth at the framebuffer's size (here: twice the clouds plane)"""
    w, h = w or 2 * c.w, h or 2 * c.h
    d = np.full((h, w), frame.cameraZNearZFar[1], f32)
    if c.depth == "wall":
        d[:, : w // 2] = f32(WALL)
    return d


def sky_plane(frame, light, size=SKY):
    """the FILL plane the CLOUDS draw samples, by sky_ref.Ref32"""
    r = sky_ref.Ref32()
    return r.fill(sc.frame_uniforms(r, frame, light), size, size)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(sky plane, clouds plane, exit steps) of a case by clouds_ref.Ref32: computed once and shared; treat as read-only"""
    c = case(name)
    sky = sky_plane(make_frame(c), c.light)
    plane, exit_step = run(cref.Ref32(), c, sky=sky)
    for a in (sky, plane, exit_step):
        a.setflags(write=False)
    return sky, plane, exit_step


def proj_view(frame):
    """projection * view as the library's host code multiplies it: what sailor_hip_sky_sun_clouds hands its kernel"""
    return host.mat4_mul(np.asarray(list(frame.projection), f32), np.asarray(list(frame.view), f32))


def alpha_plane(kind, w=64, h=48):
    """synthetic clouds planes for the sun behind clouds: rgb arbitrary, alpha straddling 0.5 across the middle of the view"""
    rng = np.random.default_rng(SEED + 1)
    p = rng.random((h, w, 4)).astype(f32)
    x, y = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
    if kind == "ramp":
        p[..., 3] = (0.5 + 6.0 * (x - 0.5) + 3.0 * (y - 0.5)).astype(f32)
    elif kind == "cells":
        p[..., 3] = ((np.arange(w)[None, :] // 2 + np.arange(h)[:, None] // 2) % 2).astype(f32)
    elif kind == "zero":
        p[..., 3] = 0.0
    else:
        raise ValueError(kind)
    return p


def run(r, c, sky=None, tex=None):
    """(clouds plane, exit steps) of a case by restatement r (clouds_ref.Ref32 or Ref64)"""
    frame, p = make_frame(c), params(c)
    U = sc.frame_uniforms(r.G, frame, c.light)
    weather, low, high, noise = tex or textures()
    C = r.context(U, p, frame.currentTime, weather, low, high, noise)
    sky = sky_plane(frame, c.light) if sky is None else sky
    return r.clouds(C, sky, depth_plane(c, frame), frame.cameraZNearZFar[1], c.w, c.h)


def coverage(c, plane, exit_step, trans_exit):
    """what a case must exercise: (texels with alpha > 0, texels that leave on transmittance, texels that return early)"""
    return int((plane[..., 3] > 0).sum()), int(trans_exit.sum()), int((exit_step == cref.EARLY).sum())


def transmittance_exits(plane, exit_step):
    """texels whose march ended with transmittanceLow < 0.05, i.e. alpha > 0.95 (:579) before the last step"""
    return (exit_step >= 0) & (exit_step < cref.RAN_OUT) & (plane[..., 3] > 0.95)


def assert_coverage(c, plane, exit_step):
    lit, gone, early = coverage(c, plane, exit_step, transmittance_exits(plane, exit_step))
    assert early > 0, (c.name, "no texel returns early")
    if c.steps == 0:
        assert lit == 0 and gone == 0, c.name   # the scattering loop never runs: alpha is 0 everywhere
        return lit, gone, early
    assert lit > 0 and gone > 0, (c.name, lit, gone, early)
    assert (plane[..., 3] > 0).sum() > gone, (c.name, "every lit texel is opaque")
    return lit, gone, early
