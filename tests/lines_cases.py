"""Named scenes for the DebugDraw pass (tests/lines_ref.py's scene dicts), each with what it was built to reach: a predicate over the restatement's result.
Frames are 16 x 12 up to 64 x 40 -- except the lane / wave hand-over cases, which need more than 64 major-axis steps and therefore a frame of 72 pixels in that
axis -- and every scene carries a band (`rows`) that is not the whole frame: the restatement is held to it on the CPU (any rows); on the device a band is whole
tile rows of 16 from the bottom (sailor_hip_band_is_valid), so the GPU test renders both bands of a two-way split of every frame taller than one tile row.

Two matrices place points exactly: IDENT (clip = (x, y, z, 1): a point is given in pixels and depth) and w_matrix(k) (clip = (x, y, k, z): the position's z is
the clip w, the depth is k / w), so that end points can sit on pixel centres and borders to the 1/256 pixel."""
import numpy as np

import lines_ref as ref

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(16)
NUM_SOUPS = 20
GOLDEN_CASES = ("diagonals_both_directions", "on_pixel_borders", "through_the_near_plane")


def w_matrix(k):
    m = np.zeros((4, 4), f32)          # m[c] = column c
    m[0][0] = 1; m[1][1] = 1
    m[2][3] = 1                        # clip.w = position.z
    m[3][2] = k                        # clip.z = k
    return m.reshape(16)


def ndc(px, py, W, H):
    return 2.0 * px / W - 1.0, 1.0 - 2.0 * py / H


def make_scene(W, H, segments, rows, vp=IDENT, indices=None, depth=None, target=None, prim_base=0):
    """segments: (a, b, colour_a, colour_b) with a, b = (px, py, z) under IDENT or (px, py, w) under a w_matrix (the point is then (nx w, ny w, w))"""
    v = np.zeros(2 * len(segments), ref.VERTEX)
    for s, (a, b, ca, cb) in enumerate(segments):
        for k, (p, c) in enumerate(((a, ca), (b, cb))):
            nx, ny = ndc(p[0], p[1], W, H)
            v["position"][2 * s + k] = (nx, ny, p[2]) if vp is IDENT else (nx * p[2], ny * p[2], p[2])
            v["color"][2 * s + k] = c
    if target is None:   # Main as a pass before left it: something a lost pixel must keep
        j, i = np.mgrid[0:H, 0:W]
        target = np.stack([i / 64.0, j / 64.0, (i + j) / 128.0, np.full_like(i, 0.75, float)], -1).astype(f32)
    return dict(W=W, H=H, vp=np.asarray(vp, f32), vertices=v, indices=None if indices is None else np.asarray(indices, np.uint32), prim_base=prim_base,
                depth=depth, target=target, rows=rows)


RED, GREEN, BLUE, WHITE = (1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 1, 0.5), (1, 1, 1, 1)


def seg(a, b, c=WHITE, c2=None, z=0.5):
    return ((a[0], a[1], a[2] if len(a) > 2 else z), (b[0], b[1], b[2] if len(b) > 2 else z), c, c if c2 is None else c2)


def owned(r):
    return {(int(i), int(j) + r["rows"][0]) for j, i in zip(*np.nonzero(r["owner"] >= 0))}


def owned_by(r, s):
    return {(int(i), int(j) + r["rows"][0]) for j, i in zip(*np.nonzero(r["owner"] == s))}


def st(r, k):
    return r["stats"].get(k, 0)


# (through_the_near_plane: the cut end, x = 11.5, is a pixel centre and excluded; through_the_far_plane: z == 0 at x = 11.5 is not > 0: both end at column 10)
# ---- the cases: name -> (builder, predicate(result of the whole-frame render, scene)) ---------------------------------------------------------------
def _horizontal():
    return make_scene(16, 12, [seg((2.5, 4.5), (9.5, 4.5), RED), seg((12.5, 7.5), (3.5, 7.5), GREEN)], (3, 9))


def _vertical():
    return make_scene(16, 12, [seg((4.5, 1.5), (4.5, 9.5), RED), seg((10.5, 10.5), (10.5, 2.5), GREEN)], (2, 11))


def _diagonals():
    c = (8.5, 6.5)
    ends = [(12.5, 10.5), (4.5, 10.5), (4.5, 2.5), (12.5, 2.5)]
    return make_scene(16, 12, [seg(c, e, RED) for e in ends] + [seg(e, c, GREEN, z=0.25) for e in ends], (1, 11))


def _octant_star():
    c = (16.5, 10.5)
    d = [(9, 0), (9, 4), (8, 8), (4, 9), (0, 9), (-4, 9), (-8, 8), (-9, 4), (-9, 0), (-9, -4), (-8, -8), (-4, -9), (0, -9), (4, -9), (8, -8), (9, -4)]
    out = [seg(c, (c[0] + x, c[1] + y), RED, BLUE) for x, y in d]
    in_ = [seg((c[0] + 1.25 * x + 0.3, c[1] + 1.25 * y - 0.2), (c[0] + 0.3, c[1] - 0.2), GREEN, WHITE, z=0.75) for x, y in d[::3]]
    return make_scene(33, 21, out + in_, (2, 19))


def _on_pixel_centres():
    return make_scene(16, 12, [seg((2.5, 2.5), (6.5, 2.5), RED), seg((6.5, 5.5), (2.5, 5.5), GREEN), seg((9.5, 2.5), (9.5, 6.5), BLUE), seg((12.5, 6.5), (12.5, 2.5))], (1, 8))


def _on_pixel_borders():
    # a horizontal segment ON the border between two rows belongs to the lower row's pixel (floor), a vertical one on a column border to the right column
    return make_scene(16, 12, [seg((2.0, 3.0), (7.0, 3.0), RED), seg((9.0, 2.0), (9.0, 8.0), GREEN), seg((2.25, 7.0), (8.25, 10.0), BLUE)], (2, 11))


def _polyline_joint():
    return make_scene(16, 12, [seg((2.5, 2.5), (7.5, 4.5), RED), seg((7.5, 4.5), (12.5, 9.5), GREEN), seg((12.5, 9.5), (3.5, 9.5), BLUE)], (1, 11))


def _one_fragment_and_none():
    return make_scene(16, 12, [seg((2.3, 2.5), (2.7, 2.6), RED),            # one pixel centre crossed
                               seg((5.6, 5.5), (5.9, 5.6), GREEN),           # none: no centre between the ends
                               seg((8.25, 8.25), (8.25, 8.25), BLUE)], (1, 10))  # zero length


def _hand_over(n):
    def build():
        return make_scene(72, 20, [seg((2.5, 3.5), (2.5 + n, 9.5), RED, BLUE), seg((2.5 + n, 14.5), (2.5, 12.5), GREEN)], (2, 17))
    return build


def _hand_over_tall():
    return make_scene(20, 72, [seg((3.5, 70.5), (12.5, 1.5), RED, BLUE), seg((15.5, 2.5), (16.5, 66.5), GREEN), seg((1.5, 2.5), (2.5, 67.5), WHITE)], (1, 71))


def _longer_than_the_frame():
    return make_scene(24, 16, [seg((-10.0, -7.0), (33.0, 24.0), RED, BLUE), seg((40.0, -3.0), (-20.0, 19.0), GREEN, WHITE, z=0.25),
                               seg((2.0, 16.0), (20.0, 16.0), WHITE)], (3, 14))   # along the lower border, inside the view volume: row 16 of 16 does not exist


def _through_the_near_plane():
    # under IDENT the near plane is z <= 1
    return make_scene(24, 16, [seg((2.5, 3.5, 0.5), (20.5, 3.5, 1.5), RED, BLUE), seg((20.5, 8.5, 1.25), (3.5, 10.5, 0.25), GREEN, WHITE),
                               seg((2.5, 12.5, 1.5), (20.5, 13.5, 1.25), BLUE)], (1, 14))


def _through_the_far_plane():
    return make_scene(24, 16, [seg((2.5, 3.5, 0.5), (20.5, 5.5, -0.5), RED, BLUE), seg((3.5, 9.5, -0.25), (20.5, 9.5, -0.5), GREEN)], (1, 14))


def _through_each_side_plane():
    return make_scene(24, 16, [seg((4.5, 3.5), (-6.5, 5.5), RED, BLUE), seg((30.5, 6.5), (18.5, 7.5), GREEN, WHITE), seg((8.5, 12.5), (9.5, 22.5), BLUE, RED),
                               seg((14.5, -5.5), (12.5, 4.5), WHITE, GREEN)], (2, 15))


def _wholly_outside():
    return make_scene(24, 16, [seg((-8.5, 3.5), (-2.5, 9.5)), seg((26.5, 3.5), (30.5, 9.5)), seg((3.5, -4.5), (20.5, -1.5)), seg((3.5, 17.5), (20.5, 19.5)),
                               seg((3.5, 4.5, 1.5), (20.5, 9.5, 2.0)),
                               # each end outside one plane, the line passes outside the corner: t_in > t_out
                               seg((-6.0, 1.6), (2.4, -4.0), RED)], (2, 13))


def _w_not_positive():
    m = np.zeros((4, 4), f32)          # clip = (x, y, 1.5 z - 1, z): a position with z == 1 has depth 0.5
    m[0][0] = 1; m[1][1] = 1; m[2][2] = 1.5; m[2][3] = 1; m[3][2] = -1
    s = make_scene(16, 12, [seg((4.5, 4.5, 1.0), (9.5, 6.5, 1.0), RED), seg((4.5, 8.5, 1.0), (9.5, 9.5, 1.0), GREEN)], (2, 11), vp=m.reshape(16))
    s["vertices"]["position"][0] = (0.0, 0.0, 0.0)    # clip (0, 0, -1, 0): inside every plane, w == 0
    return s


def _nan_and_inf_vertices():
    s = make_scene(16, 12, [seg((2.5, 2.5), (9.5, 4.5), RED), seg((2.5, 5.5), (9.5, 7.5), GREEN), seg((2.5, 8.5), (9.5, 9.5), BLUE), seg((3.5, 1.5), (12.5, 1.5))], (1, 10))
    s["vertices"]["position"][0][0] = np.nan          # (0 x NaN: the whole clip position is NaN, w too)
    s["vertices"]["position"][2][0], s["vertices"]["position"][3][0] = -3.0e38, 3.0e38   # B - A overflows: the cut end is not finite, its w is
    s["vertices"]["color"][5][1] = np.nan             # a NaN colour is drawn: the pixel gets the NaN
    return s


def _depth_tie_between_segments():
    return make_scene(16, 12, [seg((2.5, 2.5), (12.5, 9.5), RED), seg((2.5, 9.5), (12.5, 2.5), GREEN), seg((7.5, 1.5), (7.5, 10.5), BLUE)], (1, 11))


def _tie_with_the_seeded_depth():
    return make_scene(16, 12, [seg((2.5, 3.5), (12.5, 8.5), RED)], (2, 10), depth=np.full((12, 16), 0.5, f32))


def _behind_the_seeded_depth():
    d = np.full((12, 16), 0.5, f32)
    d[:, 8:] = 0.125
    return make_scene(16, 12, [seg((2.5, 3.5), (13.5, 8.5), RED, z=0.25)], (2, 10), depth=d)


def _end_colours_with_very_different_w():
    return make_scene(40, 24, [seg((3.5, 4.5, 0.5), (35.5, 18.5, 8.0), RED, BLUE), seg((35.5, 3.5, 0.375), (4.5, 20.5, 16.0), GREEN, WHITE)], (2, 22), vp=w_matrix(0.25))


def _index_buffer():
    s = make_scene(16, 12, [seg((2.5, 2.5), (12.5, 3.5), RED, GREEN), seg((3.5, 9.5), (11.5, 7.5), BLUE, WHITE)], (1, 11))
    s["indices"] = np.array([2, 0, 0, 3, 3, 3, 1, 2, 0, 1], np.uint32)
    s["prim_base"] = 1000
    return s


def _only(r, pixels):
    return owned(r) == set(pixels)


CASES = {
    "horizontal": (_horizontal, lambda r, s: _only(r, [(i, 4) for i in range(2, 9)] + [(i, 7) for i in range(4, 13)])),
    "vertical": (_vertical, lambda r, s: _only(r, [(4, j) for j in range(1, 9)] + [(10, j) for j in range(3, 11)])),
    "diagonals_both_directions": (_diagonals, lambda r, s: st(r, "major_axis_tie") == 8 and st(r, "y_major") == 0 and len(owned(r)) == 17),
    "octant_star": (_octant_star, lambda r, s: st(r, "x_major") > 4 and st(r, "y_major") > 4 and st(r, "rising") > 4 and st(r, "falling") > 4),
    "on_pixel_centres": (_on_pixel_centres, lambda r, s: owned_by(r, 0) == {(i, 2) for i in range(2, 6)} and owned_by(r, 1) == {(i, 5) for i in range(3, 7)}
                         and owned_by(r, 2) == {(9, j) for j in range(2, 6)} and owned_by(r, 3) == {(12, j) for j in range(3, 7)}),
    "on_pixel_borders": (_on_pixel_borders, lambda r, s: owned_by(r, 0) == {(i, 3) for i in range(2, 7)} and owned_by(r, 1) == {(9, j) for j in range(2, 8)}
                         and owned_by(r, 2) == {(2, 7), (3, 7), (4, 8), (5, 8), (6, 9), (7, 9)}),
    "polyline_joint_hit_once": (_polyline_joint, lambda r, s: st(r, "won_a_tie_with_a_segment") == 0 and st(r, "overwritten") == 0 and r["owner"][4, 7] == 1
                                and r["owner"][9, 12] == 2 and len(owned(r)) == 5 + 5 + 9),
    "one_fragment_and_none": (_one_fragment_and_none, lambda r, s: _only(r, [(2, 2)]) and st(r, "empty_range") == 1 and st(r, "zero_length") == 1),
    "hand_over_64": (_hand_over(64), lambda r, s: st(r, "wave_path") == 0 and st(r, "lane_path") == 2 and len(owned_by(r, 0)) == 64),
    "hand_over_65": (_hand_over(65), lambda r, s: st(r, "wave_path") == 2 and st(r, "lane_path") == 0 and len(owned_by(r, 0)) == 65 and len(owned_by(r, 1)) == 65),
    "hand_over_tall": (_hand_over_tall, lambda r, s: st(r, "wave_path") == 2 and st(r, "lane_path") == 1 and st(r, "y_major") == 3),
    "longer_than_the_frame": (_longer_than_the_frame, lambda r, s: st(r, "cut_in_left") == 1 and st(r, "cut_in_right") == 1 and len(owned(r)) > 20 and st(r, "fragments_outside") == 18),
    "through_the_near_plane": (_through_the_near_plane, lambda r, s: st(r, "cut_out_near") == 1 and st(r, "cut_in_near") == 1 and st(r, "reject_near") == 1
                               and max(i for i, j in owned_by(r, 0)) == 10),
    "through_the_far_plane": (_through_the_far_plane, lambda r, s: st(r, "fragments_beyond_depth_range") > 10 and max(i for i, j in owned(r)) == 10),
    "through_each_side_plane": (_through_each_side_plane, lambda r, s: all(st(r, k) == 1 for k in ("cut_out_left", "cut_in_right", "cut_out_bottom", "cut_in_top"))
                                and all(len(owned_by(r, k)) > 2 for k in range(4))),
    "wholly_outside": (_wholly_outside, lambda r, s: all(st(r, "reject_" + p) == 1 for p in ref.PLANES) and st(r, "reject_t_in_beyond_t_out") == 1 and not owned(r)),
    "w_not_positive": (_w_not_positive, lambda r, s: st(r, "reject_w") == 1 and owned(r) == owned_by(r, 1) and len(owned(r)) == 5),
    "nan_and_inf_vertices": (_nan_and_inf_vertices, lambda r, s: st(r, "reject_w") == 1 and st(r, "reject_not_finite") == 1 and not owned_by(r, 0) and not owned_by(r, 1)
                             and np.isnan(r["target"][r["owner"] == 2]).any()),
    "depth_tie_between_segments": (_depth_tie_between_segments, lambda r, s: st(r, "won_a_tie_with_a_segment") >= 2 and r["owner"][6, 7] == 2),
    "tie_with_the_seeded_depth": (_tie_with_the_seeded_depth, lambda r, s: st(r, "won_a_tie_with_the_seed") == 10 and len(owned(r)) == 10),
    "behind_the_seeded_depth": (_behind_the_seeded_depth, lambda r, s: st(r, "fragments_behind") == 6 and {i for i, j in owned(r)} == set(range(8, 13))),
    "end_colours_with_very_different_w": (_end_colours_with_very_different_w, lambda r, s: len(owned(r)) > 40),
    "index_buffer": (_index_buffer, lambda r, s: st(r, "zero_length") == 1 and int(r["keys"].astype(np.uint32).max()) == 1000 + 4 + 1 and len(owned_by(r, 4)) > 5),
}

# what the cases and the soups must reach between them: every clip branch, both major axes and directions, both paths of the work distribution
BRANCHES = [f"{k}_{p}" for k in ("reject", "cut_in", "cut_out") for p in ref.PLANES] + [
    "reject_t_in_beyond_t_out", "reject_w", "reject_not_finite", "zero_length", "empty_range", "x_major", "y_major", "rising", "falling", "major_axis_tie",
    "lane_path", "wave_path", "fragments_outside", "fragments_beyond_depth_range", "fragments_behind", "overwritten", "won_a_tie_with_a_segment",
    "won_a_tie_with_the_seed"]


def random_soup(seed):
    """segments between random points of a view-space box under a reversed-z perspective (depth = near / distance): through the near and the side planes,
    behind the camera, over a DepthBuffer that is seeded in places"""
    rng = np.random.default_rng(1000 + seed)
    W, H = [(16, 12), (33, 21), (64, 40), (47, 40)][seed % 4]
    n = 24 + 4 * (seed % 5)
    f, near = 1.2, 0.1
    m = np.zeros((4, 4), f32)
    m[0][0] = f * H / W; m[1][1] = -f
    m[2][3] = -1.0                    # w = -z_view
    m[3][2] = near                    # clip z = near
    v = np.zeros(2 * n, ref.VERTEX)
    p = rng.uniform([-4, -3, -9], [4, 3, 1.5], (2 * n, 3))
    short = rng.random(n) < 0.4       # some short segments
    p[1::2][short] = p[0::2][short] + rng.uniform(-0.4, 0.4, (int(short.sum()), 3))
    v["position"] = p.astype(f32)
    v["color"] = rng.uniform(0, 1, (2 * n, 4)).astype(f32)
    depth = np.where(rng.random((H, W)) < 0.4, rng.uniform(0.0, 0.06, (H, W)), 0.0).astype(f32)
    target = rng.uniform(0, 1, (H, W, 4)).astype(f32)
    idx = None
    if seed % 3 == 1:
        idx = rng.integers(0, 2 * n, 2 * n).astype(np.uint32)
    r0 = 1 + seed % 3
    return dict(W=W, H=H, vp=m.reshape(16), vertices=v, indices=idx, prim_base=seed * 77, depth=depth, target=target, rows=(r0, H - 2 - seed % 2))


def all_scenes():
    s = {name: build() for name, (build, _) in CASES.items()}
    for seed in range(NUM_SOUPS):
        s[f"soup_{seed}"] = random_soup(seed)
    return s
