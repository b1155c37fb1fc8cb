"""Inputs shared by the star and sun-shaft tests, and helpers that run a restatement of tests/stars_ref.py on a case.

Fixtures (tests/golden): BSC5, the Bright Star Catalogue as the node reads it (9 110 stars; the spectral bytes ' ' and 'p' and the sub-type bytes
m p e N I C + / and space are all in it), and stars_color_rows.npy, the 782 `colors` rows of StarsColor.yaml as float32 [782, 11].

Targets are 96 x 64 and 131 x 77 (131 = 2 * 64 + 3 columns, 77 = 19 * 4 + 1 rows: partial blocks in both directions), clouds planes 32^2 and 38^2.

Sun-shaft cases.  uvView = (clip + 1) / 2 / w of dirToSun; the synthetic camera looks down -Z.  `in_view`: the sun inside the frame; every texel walks towards
it in steps of 5 / 38 of its distance and, with 60 or 100 taps, far past it, so that taps are clamped at all four edges.  `fading`: the sun to the right of the
frame, 1 < uvView.x < 1.51: fade > 0 and the mix term below 1.  `behind`: dirToSun behind the camera, a small positive w, uvView far outside: the second
uniform early-out.  `dark`: sunShaftsIntensity = 0, the first.  sunShaftsDistance takes 1, 7, 60 and 100.

Star cases.  `fixture_*`: the catalogue's mesh under sailor_host_sky_stars_model; the camera stands 1 150 m above the ground in the fragment shader's units
(origin = (0, R + 1000, 0) + cameraPosition, no 0.01), so the horizon lies 1.09 degrees below level and the stars of the lower rows are on Earth-hitting
rays.  `synthetic_*`: 64 stars placed by unprojecting pixel positions in float64 (model = identity): four on one pixel, three on its neighbour, three on a
pixel below the horizon, one on the view axis (the corner of four pixels where w and h are even), one behind the camera, one off each side of the clip
volume, one nearer than zNear and one beyond zFar, one with a NaN and one with an infinite position, the rest scattered over a 6 x 3 block of pixels within
1e-4 of the pixel centres so that they collide and are lit.  `empty`: count = 0.
"""
import functools
from collections import namedtuple
from pathlib import Path

import numpy as np

import clouds_cases as cc
import sky_cases as sc
import stars_ref as sref
from sailor_amd import host

f32 = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
SEED = 20240902

ShaftCase = namedtuple("ShaftCase", "name w h cw light pitch distance intensity kind")
SHAFT_CASES = [
    ShaftCase("in_view_60", 96, 64, 32, (0.0, -0.1, 1.0), 0.0, 60, 0.45, "in_view"),
    ShaftCase("in_view_100", 131, 77, 38, (0.3, -0.25, 1.0), 10.0, 100, 0.45, "in_view"),
    ShaftCase("in_view_1", 131, 77, 32, (-0.2, -0.3, 1.0), 10.0, 1, 2.0, "in_view"),
    ShaftCase("fading_7", 96, 64, 38, (-1.8, -0.1, 1.0), 0.0, 7, 0.45, "fading"),
    ShaftCase("behind_60", 96, 64, 32, (0.0, -0.5, -1.0), 0.0, 60, 0.45, "behind"),
    ShaftCase("dark_100", 131, 77, 38, (0.0, -0.1, 1.0), 0.0, 100, 0.0, "dark"),
]
StarCase = namedtuple("StarCase", "name w h cw stars position pitch fov plane")
STAR_CASES = [
    StarCase("fixture_96", 96, 64, 32, "fixture", (0.0, 150.0, 0.0), 10.0, 90.0, "cells"),
    StarCase("fixture_131", 131, 77, 38, "fixture", (300.0, 150.0, -200.0), -5.0, 60.0, "ramp01"),
    StarCase("synthetic_96", 96, 64, 38, "synthetic", (0.0, 150.0, 0.0), 10.0, 90.0, "ramp01"),
    StarCase("synthetic_131", 131, 77, 32, "synthetic", (300.0, 150.0, -200.0), 10.0, 60.0, "cells"),
    StarCase("empty_96", 96, 64, 32, "empty", (0.0, 150.0, 0.0), 10.0, 90.0, "cells"),
]
SYNTHETIC_COUNT = 64
PIXEL_A, PIXEL_B, PIXEL_EARTH = (40, 20), (41, 20), (30, 60)   # four stars, three stars, three stars under the horizon


def shaft_case(name):
    return next(c for c in SHAFT_CASES if c.name == name)


def star_case(name):
    return next(c for c in STAR_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def catalogue():
    return (GOLDEN / "BSC5").read_bytes()


@functools.lru_cache(maxsize=None)
def color_rows():
    a = np.load(GOLDEN / "stars_color_rows.npy")
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def fixture_mesh():
    """(positions [9110, 3], colours [9110, 4], divisors) by Ref32; read-only"""
    r = sref.Ref32()
    out = r.star_mesh(catalogue(), r.color_table(color_rows()))
    for a in out:
        a.setflags(write=False)
    return out


def clouds_plane(kind, n):
    """an n x n clouds plane: rgb random in [0, 1) (g feeds pow(g, 3)), alpha a ramp or 2 x 2 cells of 0 and 1"""
    p = cc.alpha_plane("cells" if kind == "cells" else "ramp", n, n)
    if kind == "ramp01":
        p[..., 3] = np.clip(p[..., 3], 0.0, 1.0)
    return p


def shaft_target(c, hostile=True):
    """the `Sky` target before the pass: colours of a few units, alpha 0 as the tree stores it except for a block of other alphas; one hostile texel"""
    rng = np.random.default_rng(SEED + 3)
    t = (rng.random((c.h, c.w, 4)) * 8.0).astype(f32)
    t[..., 3] = 0.0
    t[5:15, 10:40, 3] = rng.random((10, 30)).astype(f32) * 1.5
    if hostile:
        t[2, 3] = (np.inf, -np.inf, np.nan, 0.25)
    return t


def shaft_frame(c):
    return sc.make_frame(c.w, c.h, (0.0, 150.0, 0.0), c.pitch, 90.0)


def shaft_params(c, **overrides):
    v = dict(lightDirection=c.light, sunShaftsDistance=c.distance, sunShaftsIntensity=c.intensity)
    v.update(overrides)
    return host.sky_params(**v)


def run_shafts(r, c, rows=None, target=None):
    """(blended rows, info, uniforms) of a case by restatement r"""
    U = r.shaft_uniforms(shaft_frame(c), shaft_params(c), c.cw, c.cw)
    t = shaft_target(c) if target is None else target
    j0, j1 = (0, c.h) if rows is None else rows
    out, info = r.sun_shafts(U, clouds_plane("ramp01", c.cw), t[j0:j1], c.w, c.h, rows)
    return out, info, U


@functools.lru_cache(maxsize=None)
def shaft_reference(name):
    out, info, U = run_shafts(sref.Ref32(), shaft_case(name))
    out.setflags(write=False)
    return out, info, U


def star_frame(c):
    return sc.make_frame(c.w, c.h, c.position, c.pitch, c.fov)


def synthetic_stars(frame, w, h):
    """64 stars by unprojection in float64 -> (positions float32 [64, 3], colours float32 [64, 4])"""
    rng = np.random.default_rng(SEED + 4)
    inv_proj = np.linalg.inv(np.asarray(list(frame.projection), np.float64).reshape(4, 4).T)
    inv_view = np.linalg.inv(np.asarray(list(frame.view), np.float64).reshape(4, 4).T)

    def at_pixel(sx, sy, depth=0.5):
        clip = np.array([2.0 * sx / w - 1.0, 1.0 - 2.0 * sy / h, depth, 1.0])
        v = inv_proj @ clip
        return (inv_view @ (v / v[3]))[:3]

    def in_view_space(x, y, z):
        return (inv_view @ np.array([x, y, z, 1.0]))[:3]

    pos = []
    ax, ay = PIXEL_A
    pos += [at_pixel(ax + 0.5, ay + 0.5), at_pixel(ax + 0.53, ay + 0.5), at_pixel(ax + 0.2, ay + 0.7), at_pixel(ax + 0.5, ay + 0.5, 0.25)]
    bx, by = PIXEL_B
    pos += [at_pixel(bx + 0.5 + d, by + 0.5 - d) for d in (0.0, 0.01, 0.02)]
    ex, ey = PIXEL_EARTH
    pos += [at_pixel(ex + 0.5, ey + 0.5, z) for z in (0.3, 0.5, 0.7)]
    pos.append(in_view_space(0.0, 0.0, -1000.0))                          # the view axis: ndc = 0 exactly
    pos.append(in_view_space(10.0, 20.0, 1000.0))                         # behind the camera: w <= 0
    pos += [at_pixel(-0.25 * w, 0.5 * h), at_pixel(1.25 * w, 0.5 * h), at_pixel(0.5 * w, 1.25 * h), at_pixel(0.5 * w, -0.25 * h)]   # x low, x high, y low, y high
    pos += [in_view_space(0.0, 0.0, -0.5), in_view_space(0.0, 0.0, -30000.0)]   # nearer than zNear, beyond zFar
    pos += [np.array([np.nan, 0.0, -100.0]), np.array([np.inf, 0.0, -100.0])]
    while len(pos) < SYNTHETIC_COUNT:
        px, py = 50 + int(rng.integers(6)), 10 + int(rng.integers(3))
        pos.append(at_pixel(px + 0.5 + rng.uniform(-0.01, 0.01), py + 0.5 + rng.uniform(-0.01, 0.01), rng.uniform(0.2, 0.8)))
    col = rng.random((SYNTHETIC_COUNT, 4)).astype(f32)
    col[:, 3] = 1.0
    return np.asarray(pos, np.float64).astype(f32), col


@functools.lru_cache(maxsize=None)
def star_inputs(name):
    """(frame, model, positions, colours, clouds plane, target) of a case; the arrays are read-only"""
    c = star_case(name)
    frame = star_frame(c)
    if c.stars == "fixture":
        positions, colors = fixture_mesh()[:2]
        model = host.sky_stars_model(list(frame.cameraPosition)[:3])
    elif c.stars == "synthetic":
        positions, colors = synthetic_stars(frame, c.w, c.h)
        model = np.eye(4, dtype=f32).reshape(-1)
    else:
        positions, colors, model = np.zeros((0, 3), f32), np.zeros((0, 4), f32), np.eye(4, dtype=f32).reshape(-1)
    rng = np.random.default_rng(SEED + 5)
    target = (rng.random((c.h, c.w, 4)) * 0.5).astype(f32)
    target[..., 3] = 0.0
    target[3 * c.h // 4:, :, :] = -0.0   # under the horizon: -0 + 0 = +0 shows where a star's (0, 0, 0, 0) fragment was added
    plane = clouds_plane(c.plane, c.cw)
    for a in (positions, colors, model, target, plane):
        a.setflags(write=False)
    return frame, model, positions, colors, plane, target


def run_stars(r, c, rows=None, clouds=True):
    """(blended rows, per-star record) of a case by restatement r"""
    frame, model, positions, colors, plane, target = star_inputs(c.name)
    j0, j1 = (0, c.h) if rows is None else rows
    return r.stars(frame, model, positions, colors, plane if clouds else None, target[j0:j1], c.w, c.h, rows)


@functools.lru_cache(maxsize=None)
def star_reference(name):
    out, S = run_stars(sref.Ref32(), star_case(name))
    out.setflags(write=False)
    return out, S


def stars_per_pixel(S, w):
    """{pixel id: number of drawn stars on it}"""
    ids = (S["py"] * w + S["px"])[S["drop"] == 0]
    u, n = np.unique(ids, return_counts=True)
    return dict(zip(u.tolist(), n.tolist()))
