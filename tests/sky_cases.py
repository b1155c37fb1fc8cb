"""Inputs shared by the sky tests: cameras, suns and viewport sizes, and helpers that run a restatement of tests/sky_ref.py on a case.

Every case is (name, viewport w, viewport h, camera position in centimetres, pitch in degrees, lightDirection, vertical field of view).  dirToSun = -lightDirection; the
synthetic camera looks down -Z, so a sun "in view" has lightDirection.z > 0.  Heights: cameraPosition.y = 0, 150 (synth.make_camera) and 30 000 cm."""
import math
from collections import namedtuple

import numpy as np

import sky_ref as ref
from sailor_amd import host, synth

f32 = np.float32
SUN_HIGH = (0.2, -1.0, 0.3)
SUN_DEFAULT = (0.0, -1.0, 1.0)       # SkyNode.h:50 before normalisation: 45 degrees up, straight ahead
SUN_LOW_AHEAD = (0.0, -0.1, 1.0)     # 5.7 degrees above the horizon, inside the level camera's view
SUN_LOW_UP = (0.0, -0.5, 1.0)        # inside the view of the camera pitched up
SUN_BELOW = (0.0, 0.2, 1.0)          # 11 degrees under the horizon
SUN_BEHIND = (0.0, -0.5, -1.0)       # behind the camera: outside every compose window

Case = namedtuple("Case", "name w h position pitch light fov")
CASES = [
    Case("level_synth", 48, 32, (0.0, 150.0, 0.0), 0.0, SUN_DEFAULT, 90.0),            # synth.make_camera, level with the horizon
    Case("up_low_sun", 48, 32, (0.0, 150.0, 0.0), 30.0, SUN_LOW_UP, 90.0),             # pitched up, the Earth in the lower rows
    Case("down_high", 48, 32, (0.0, 30000.0, 0.0), -30.0, SUN_HIGH, 90.0),             # pitched down from 300 m
    Case("level_high_night", 48, 32, (1000.0, 30000.0, -2000.0), 0.0, SUN_BELOW, 90.0),
    Case("zenith_ground", 48, 32, (0.0, 0.0, 0.0), 60.0, SUN_HIGH, 90.0),              # height 0, sky only (see test_sky_cpu.py on why)
    Case("wide_low_sun", 640, 240, (0.0, 150.0, 0.0), 0.0, SUN_LOW_AHEAD, 90.0),       # non-square, the sun a few pixels wide
    Case("tele_sun", 48, 32, (0.0, 150.0, 0.0), math.degrees(math.atan(0.1)), SUN_LOW_AHEAD, 10.0),   # the sun dead centre of a 10 degree lens
    Case("level_sun_behind", 48, 32, (0.0, 150.0, 0.0), 0.0, SUN_BEHIND, 90.0),
]
COMPOSE_SUN_INSIDE = ("wide_low_sun", "tele_sun")
COMPOSE_SUN_OUTSIDE = ("level_sun_behind", "down_high")
ENV_CASES = [("env_default", (0.0, 150.0, 0.0), SUN_DEFAULT), ("env_low_high", (0.0, 30000.0, 0.0), SUN_LOW_AHEAD)]
SKY, SUN, FACE = 32, 8, 16           # plane sizes of the CPU comparisons and of the golden file


def case(name):
    return next(c for c in CASES if c[0] == name)


def make_frame(w, h, position, pitch_degrees, fov=90.0):
    """synth.make_camera's lens (1 .. 20000) at `position`, pitched about +X (positive = up)"""
    a = math.radians(pitch_degrees) / 2.0
    world = host.transform_matrix([position[0], position[1], position[2], 1.0], [math.sin(a), 0.0, 0.0, math.cos(a)], [1.0, 1.0, 1.0, 1.0])
    if pitch_degrees == 0.0 and tuple(position) == (0.0, 150.0, 0.0) and fov == 90.0:
        return synth.make_camera(w, h).frame
    return host.fill_frame_data(world, fov, 1.0, 20000.0, w, h)


def frame_uniforms(r, frame, light):
    return ref.uniforms_from_frame(r, frame, ref.inv_view_for(r, list(frame.view)), light)


def face_uniforms(r, face, position, light):
    view, _, inv_projection = host.sky_face_matrices(face)
    return r.uniforms(view, inv_projection, ref.inv_view_for(r, view), position, light)


def planes(r, c, sky=SKY, sun=SUN):
    """(sky, sun, compose) of a case by restatement r"""
    U = frame_uniforms(r, make_frame(c.w, c.h, c.position, c.pitch, c.fov), c.light)
    s, d = r.fill(U, sky, sky), r.sun(U, sun, sun)
    return s, d, r.compose(U, s, d, c.w, c.h)


def sun_window_changes(r, U, sky, composed, w, h):
    """does COMPOSE differ from the plain sky fetch anywhere, i.e. is the sun window in view and lit"""
    plain = r._bilinear(r.arr(sky), *r.texcoords(w, h), True)
    return bool(np.any(np.ascontiguousarray(composed[..., :3]) != plain))


def classes(a):
    """0 = zero, 1 = finite non-zero, 2 = +inf, 3 = -inf, 4 = NaN"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 4, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, np.where(a == 0, 0, 1)))).astype(np.uint8)
