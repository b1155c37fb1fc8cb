"""The scenes of the multisampled-pass tests (tests/test_msaa_cpu.py, tests/test_msaa_gpu.py), built from tests/surface_cases.py's helpers on its frames
(40 x 24 and the like).  `screen` scenes put a vertex (x, y) on the 1/256 grid at exactly x, y, so an edge can be laid between two named samples of a pixel.

The cases were built to reach, between them (tests/test_msaa_cpu.py asserts it from the restatement alone): every weight 1 .. 7 at eight samples, a pixel with
eight distinct owners (which clips at two layers), a pixel whose centre is uncovered while a cutout draw owns a sample of it -- one that keeps and one that
discards --, a triangle the near plane cut on an edge pixel, a sliver that covers samples and no centre, and a large triangle (the wave-cooperative walk)."""
import numpy as np

import surface_cases as sc
from surface_cases import draw, quad, scene, screen_projection

f32 = np.float32
W, H = 40, 24


def rect(x0, y0, x1, y1, z=0.5, **kw):
    v, t = quad(x0, y0, x1, y1, z=z, **kw)
    return draw(v, t)


def cutout(d):
    return dict(d, alpha_cutout=True)


def edge_rect(k=20, frac=128, left=False):
    """a rectangle over rows 3 .. 8 whose vertical edge is at x = k + frac / 256: its right edge, or (left) its left edge"""
    x = k + frac / 256.0
    return scene(W, H, screen_projection(W, H), [rect(x, 3.0, 30.0, 9.0) if left else rect(10.0, 3.0, x, 9.0)])


def shared_edge_rects(k=20, frac=144):
    """two rectangles, two draws, sharing the vertical edge at x = k + frac / 256, the right one nearer"""
    x = k + frac / 256.0
    return scene(W, H, screen_projection(W, H), [rect(10.0, 3.0, x, 9.0, z=0.4), rect(x, 3.0, 30.0, 9.0, z=0.6)])


def staircase():
    """seven rectangles, one a pair of rows, whose right edge is at 20 + m / 8, m = 1 .. 7: the sample columns of the eight-sample table are 32 apart from 16
    on, so the rectangle owns exactly m samples of column 20"""
    return scene(W, H, screen_projection(W, H), [rect(10.0, 2.0 + 3 * (m - 1), 20.0 + m / 8.0, 4.0 + 3 * (m - 1), z=0.3 + 0.05 * m) for m in range(1, 8)])


def eight_owners():
    """eight strips an eighth of a pixel wide over column 20, one draw each: every sample of a pixel of that column has an owner of its own"""
    return scene(W, H, screen_projection(W, H), [rect(20.0 + m / 8.0, 2.5, 20.0 + (m + 1) / 8.0, 10.5, z=0.3 + 0.05 * m) for m in range(8)])


def cutout_at_the_edge():
    """two cutout rectangles whose right edge, at 20 + 100 / 256, lies left of column 20's centre: the samples at 16, 48 and 80 are inside, the centre is not.
    The vertex colour's alpha falls from 0.9 at x = 10 to `a` at the edge: the upper rectangle (a = 0.6) is still above one half at the centre, where the
    shader runs, and keeps; the lower (a = 0.502) is above one half at every sample it covers and below it at the centre, and is discarded there.
    An opaque rectangle behind both shows through where they discard."""
    x = 20.0 + 100.0 / 256.0

    def faded(y0, y1, a):
        return cutout(rect(10.0, y0, x, y1, z=0.6, colors=[(1, 1, 1, 0.9), (1, 1, 1, a), (1, 1, 1, a), (1, 1, 1, 0.9)]))
    return scene(W, H, screen_projection(W, H), [rect(5.0, 1.0, 35.0, 20.0, z=0.2), faded(3.0, 8.0, 0.6), faded(11.0, 16.0, 0.502)])


def sliver_between_centres():
    """a rectangle inside pixel (20, 10), right of and above its centre: it holds the samples (144, 80) and (240, 16) of eight, and no centre"""
    return scene(W, H, screen_projection(W, H), [rect(20.55, 10.05, 20.95, 10.45)])


def prepass_scene():
    """two overlapping rectangles and a strip, for the pass begun from its own sample depths"""
    return scene(W, H, screen_projection(W, H), [rect(4.3, 2.2, 25.6, 15.7, z=0.4), rect(14.1, 8.3, 36.4, 21.8, z=0.7), rect(20.125, 1.0, 20.375, 23.0, z=0.5)])


def high_orders():
    """shared_edge_rects under the largest primBase its two draws allow (each adds 4 orders: two triangles, two parts): the last triangle's orderPlus1 is
    2^32 - 3, at the unsigned end of the key's low word"""
    s = shared_edge_rects()
    s["prim_base"] = 2 ** 32 - 2 - 8
    return s


CASES = {
    "edge_rect_left_128": lambda: edge_rect(20, 128, left=True),
    "edge_rect_left_144": lambda: edge_rect(20, 144, left=True),
    "edge_rect_right_144": lambda: edge_rect(20, 144),
    "shared_edge_rects": shared_edge_rects,
    "staircase": staircase,
    "eight_owners": eight_owners,
    "cutout_at_the_edge": cutout_at_the_edge,
    "sliver_between_centres": sliver_between_centres,
    "prepass_scene": prepass_scene,
    "high_orders": high_orders,
    "shared_edge_quad": sc.shared_edge_quad,
    "fan_around_a_pixel_centre": sc.fan_around_a_pixel_centre,
    "tie_two_draws": sc.tie_two_draws,
    "near_plane": sc.near_plane,
    "instance_indirection": sc.instance_indirection,
    "triangle_larger_than_the_frame": sc.triangle_larger_than_the_frame,
    "degenerates": sc.degenerates,
    "soup_3": lambda: sc.random_soup(3),
    "soup_8": lambda: sc.random_soup(8),
}
BAND_CASES = ("staircase", "near_plane", "triangle_larger_than_the_frame")


def constant_target(s, value=(0.25, 0.5, 0.125, 1.0)):
    return np.broadcast_to(np.array(value, f32), (s["H"], s["W"], 4)).copy()
