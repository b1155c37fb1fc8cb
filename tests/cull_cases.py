"""Constructed scenes for the tile light cull (ComputeLightCulling.shader:119-240, Math.glsl:224-239), shared by tests/test_cull_cpu.py (the C oracle
against the NumPy restatement and against float64) and tests/test_cull_gpu.py (every path of sailor_amd/csrc/light_cull.hip against the C oracle).
Pure NumPy.  The lists are bit for bit or wrong: nothing here carries a tolerance.

What the synthetic light sets never do is put a sphere within a few floats of a comparison.  These scenes do, and they do it on the fp32 OPERAND: a
light's view position is evaluated exactly as the oracle evaluates it (oracle_np.view_positions), the plane distance d (or the depth bound) exactly
as the oracle evaluates it, and the radius is then set to that float, the float above and the float below -- tangency is exact in fp32 whatever the
view transform rounds.  The constructed lights take the LOWEST light indices (only a tile's first 196 candidates in index order reach its list: a
wrongly dropped light further back would be invisible), filler follows, and N >= 512 unless a case is about the brute-force walk.

Frames: 256 x 192 (4 x 3 groups of 4 x 4 tiles), 131 x 77 (ragged: the last group column is one tile wide, the last group row one tile high, both
reach past the viewport), and the special shapes of the `wide_forms`.  The camera sits at (0, 150, 0) with the identity rotation.

coverage(name) counts what a case reaches from the fp32 / float64 tables alone -- never from what the builder meant to place -- and `Case.expect`
names the counts a case exists for, with the least value each must have."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle, oracle_np
from sailor_amd import host, synth

F = np.float32
TILE, GROUP, CAND, KEEP, CAPG = 16, 4, 196, 128, 2048
BIG, RAGGED = (256, 192), (131, 77)
MARGIN = F(1e-3)                              # light_cull.hip's planeMargin
RANKS = ((0, 2), (1, 2), (0, 3), (1, 3), (2, 3))   # the bands (rank, world size) every case is also culled on


@dataclass
class Case:
    cam: synth.Camera
    depth: np.ndarray                         # float32[H, W] linear depth: what the oracle gets
    lights: np.ndarray
    expect: dict = field(default_factory=dict)   # coverage name -> least count
    raw_depth: np.ndarray | None = None       # the reversed-Z image whose oracle.linearize_depth IS `depth` (SAILOR_CULL_RAW_DEPTH)
    constructed: int = 0                      # the lights [0, constructed) are the placed ones
    notes: dict = field(default_factory=dict)

    @property
    def size(self):
        return self.cam.width, self.cam.height


# ---- floats -------------------------------------------------------------------------------------------------------------------------------------
def ordinal(a) -> np.ndarray:
    """int64, monotone in the float32 value: adjacent floats differ by 1, -0.0 and +0.0 are both 0 (NaNs land beyond the infinities)"""
    b = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def up(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, F(np.inf))
    return x


def down(x, n=1):
    x = F(x)
    for _ in range(n):
        x = np.nextafter(x, F(-np.inf))
    return x


# ---- geometry of a frame ------------------------------------------------------------------------------------------------------------------------
class Geo:
    """the frame's matrices and the view-space rays of screen points (float64: only used to PLACE a light; what decides is evaluated in fp32)"""

    def __init__(self, cam):
        self.cam = cam
        self.fb = bytes(cam.frame)
        self.view, self.inv, self.vp_w, self.vp_h = oracle_np._frame_fields(self.fb)
        self.inv64 = self.inv.astype(np.float64)
        self.W, self.H = cam.width, cam.height
        self.Tx, self.Ty = (self.W - 1) // TILE + 1, (self.H - 1) // TILE + 1
        self.world = cam.world.reshape(4, 4).astype(np.float64)        # world[c] = column c

    def ray(self, sx, sy):
        """view-space direction (x, y, z) of screen point (sx, sy), z = +1 in front of the eye"""
        v = oracle_np._screen_to_view(self.inv64, sx, sy, -1.0, 1.0, self.vp_w, self.vp_h, np.float64)
        return v / v[2]

    def to_world(self, pv):
        """view-space (x, y, z in front) -> world position float32[3]"""
        x, y, z = pv
        return (self.world[0, :3] * x + self.world[1, :3] * y + self.world[2, :3] * (-z) + self.world[3, :3]).astype(F)

    @functools.lru_cache(maxsize=None)
    def rect_planes(self, rect, dtype=F):
        planes, _, _ = oracle_np.rect_frustum(self.inv.astype(dtype), *rect, self.vp_w, self.vp_h, dtype)
        return np.stack(planes)

    def tile_rect(self, tx, ty):
        return (tx * TILE, ty * TILE, (tx + 1) * TILE, (ty + 1) * TILE)

    def tile_depth(self, depth, tx, ty):
        lx = np.arange(TILE)
        rows = np.clip(self.H - 1 - (TILE * ty + lx), 0, self.H - 1)
        cols = np.minimum(TILE * tx + lx, self.W - 1)
        return depth[np.ix_(rows, cols)]

    def band_rows(self, rank_of):
        if rank_of is None:
            return 0, self.Ty
        b = host.band_for_rank(self.W, self.H, *rank_of)
        return b.tileRowBegin, b.tileRowEnd

    def group_rects(self, rows):
        """the rectangles k0_lights builds for a band of tile rows [r0, r1): (group columns, group rows), as light_cull.hip:226 and :232 state them"""
        r0, r1 = rows
        gx = (self.Tx + GROUP - 1) // GROUP
        gy = (r1 - r0 + GROUP - 1) // GROUP
        cols = [(b * GROUP * TILE, 0, min((b + 1) * GROUP, self.Tx) * TILE, self.Ty * TILE) for b in range(gx)]
        rws = [(0, (r0 + g * GROUP) * TILE, self.Tx * TILE, (r0 + min((g + 1) * GROUP, r1 - r0)) * TILE) for g in range(gy)]
        return cols, rws

    def select_rect(self, rows):
        """k0_band_count's rectangle: the whole band"""
        return (0, rows[0] * TILE, self.Tx * TILE, rows[1] * TILE)


def blank_lights(n, kind=host.LIGHT_POINT):
    L = np.zeros(n, host.LIGHT_DTYPE)
    L["type"] = kind
    L["shadowType"] = host.SHADOW_NONE
    L["intensity"] = F(1.0)
    L["attenuation"] = np.array([1.0, 0.022, 0.0019], F)
    L["direction"] = np.array([0.0, -1.0, 0.0], F)
    L["bounds"] = F(1.0)
    return L


def cat(parts):
    """the records of `parts` in one array of host.LIGHT_DTYPE (np.concatenate would pack the padded record)"""
    out = np.zeros(sum(len(p) for p in parts), host.LIGHT_DTYPE)
    at = 0
    for p in parts:
        for f in host.LIGHT_DTYPE.names:
            out[f][at:at + len(p)] = p[f]
        at += len(p)
    return out


def set_radius(L, j, r):
    L["bounds"][j] = np.asarray(r, F)[..., None] if np.ndim(r) else F(r)


def plane_d(pl, px, py, pz):
    """the fp32 distance of Math.glsl:224-239, in the oracle's op order"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (pl[0] * px + pl[1] * py) + pl[2] * pz


def outside_point(geo, depth, tile, k, rng, s_rel, z=None):
    """a view-space point outside plane k (0 left, 1 right, 2 top, 3 bottom) of `tile` by s_rel tile widths, beside the middle part of that edge,
    at the tile's own depth -- so the tile's other five comparisons accept a sphere there whatever its radius"""
    tx, ty = tile
    x0, y0, x1, y1 = geo.tile_rect(tx, ty)
    u = 0.25 + 0.5 * rng.random()
    sx, sy = {0: (x0, y0 + u * TILE), 1: (x1, y0 + u * TILE), 2: (x0 + u * TILE, y0), 3: (x0 + u * TILE, y1)}[k]
    if z is None:
        td = geo.tile_depth(depth, tx, ty).astype(np.float64)
        z = 0.5 * (td.min() + td.max())
    n = geo.rect_planes(geo.tile_rect(tx, ty), np.float64)[k]
    width = abs(geo.ray(x1, y0)[0] - geo.ray(x0, y0)[0]) * z
    return geo.ray(sx, sy) * z - s_rel * width * n


def spread_tiles(geo, rng, count):
    """tiles for the constructed lights: the four corners, the (ragged) last column and last row, then interior tiles"""
    Tx, Ty = geo.Tx, geo.Ty
    tiles = [(0, 0), (Tx - 1, 0), (0, Ty - 1), (Tx - 1, Ty - 1)]
    tiles += [(Tx - 1, y) for y in range(1, Ty - 1)] + [(x, Ty - 1) for x in range(1, Tx - 1)]
    inner = [(x, y) for y in range(1, max(Ty - 1, 2)) for x in range(1, max(Tx - 1, 2)) if x < Tx and y < Ty]
    order = rng.permutation(len(inner))
    tiles += [inner[i] for i in order]
    return [tiles[i % len(tiles)] for i in range(count)]


def filler(cam, depth, count, seed, **kw):
    cfg = dict(spot_fraction=0.3, radius_scale=3.0)
    cfg.update(kw)
    return synth.make_lights(cam, depth, synth.LightSetConfig(count=count, **cfg), seed) if count > 0 else blank_lights(0)


def far_filler(geo, count, rng):
    """cheap filler: small spheres far to the side of the frustum, in front of the eye (every tile rejects them by a side plane, by a wide margin)"""
    L = blank_lights(count)
    z = 50.0 + 400.0 * rng.random(count)
    edge = abs(geo.ray(0.0, 0.0)[0])
    x = (3.0 + 5.0 * rng.random(count)) * edge * z * np.where(rng.random(count) < 0.5, -1.0, 1.0)
    y = (2.0 * rng.random(count) - 1.0) * z
    w = geo.world
    L["worldPosition"] = (w[0, :3][None] * x[:, None] + w[1, :3][None] * y[:, None] + w[2, :3][None] * (-z)[:, None] + w[3, :3][None]).astype(F)
    L["bounds"] = (0.01 * z).astype(F)[:, None]
    return L


def make_cam(size, fov=90.0, view="affine"):
    cam = synth.make_camera(size[0], size[1], fov=fov)
    if view == "scaled":                       # all sixteen entries of frame.view doubled: w == 2 in every lane, p / w unchanged
        f = host.fill_frame_data(cam.world, cam.fov, cam.z_near, cam.z_far, cam.width, cam.height)
        for i in range(16):
            f.view[i] = f.view[i] * 2.0
        cam = synth.Camera(world=cam.world, fov=cam.fov, z_near=cam.z_near, z_far=cam.z_far, width=cam.width, height=cam.height, frame=f)
    return cam


def fov_for(p, aspect=1.0):
    """the vertical field of view (degrees) whose projection has p = 1 / (aspect tan(fov / 2))"""
    return float(np.degrees(2.0 * np.arctan(1.0 / (p * aspect))))


# ---- tile_planes --------------------------------------------------------------------------------------------------------------------------------
def tangent_lights(geo, depth, specs, rng):
    """specs: (tile, plane k, radius class c, s_rel) per light; the light's radius is -d (c = 0: d == -r, listed), the float above (c = +1: listed)
    or the float below (c = -1: d < -r, dropped), d being the fp32 distance of the light's fp32 view position from the TILE's own plane k"""
    L = blank_lights(len(specs))
    for j, (tile, k, c, s_rel) in enumerate(specs):
        L["worldPosition"][j] = geo.to_world(outside_point(geo, depth, tile, k, rng, s_rel))
    px, py, pz = oracle_np.view_positions(geo.fb, L)
    for j, (tile, k, c, s_rel) in enumerate(specs):
        pl = geo.rect_planes(geo.tile_rect(*tile))[k]
        r = -plane_d(pl, px[j], py[j], pz[j])
        assert r > 0 and np.isfinite(r), (tile, k, r)
        set_radius(L, j, r if c == 0 else (up(r) if c > 0 else down(r)))
    return L


PLANE_EXPECT = {f"plane{k}_{c}": 32 for k in range(4) for c in ("eq", "above", "below")}


def tile_planes(size, per=36, total=768, fov=90.0, view="affine", seed=1, expect=None) -> Case:
    """Spheres in front of the eye, outside one plane of some tile and tangent to it in fp32: `per` lights for each of the four planes and each
    radius class, half of them a fraction of a tile away from the plane (small spheres, centre in the neighbouring tile -- or, for a tile on the
    frame's edge, just outside the frustum), half several tiles away (large spheres)."""
    cam = make_cam(size, fov, view)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    depth = synth.make_linear_depth(size[0], size[1], seed)
    combos = [(k, c) for k in range(4) for c in (0, 1, -1)]
    tiles = spread_tiles(geo, rng, per * len(combos))
    specs = []
    for i in range(per):
        for q, (k, c) in enumerate(combos):
            s_rel = (0.05 + 0.9 * rng.random()) if i % 2 == 0 else (2.0 + 6.0 * rng.random())
            specs.append((tiles[i * len(combos) + q], k, c, s_rel))
    L = tangent_lights(geo, depth, specs, rng)
    lights = cat([L, filler(cam, depth, total - len(L), seed)]) if total > len(L) else L[:total]
    return Case(cam, depth, lights, dict(PLANE_EXPECT, fp32_ne_fp64=1) if expect is None else expect, constructed=min(len(L), total))


# ---- band_edges / margin_window -----------------------------------------------------------------------------------------------------------------
def edge_tiles(geo, rows, axis):
    """(tile, plane k, band rectangle) for every band-edge plane of the band of tile rows `rows`: the tile lies on the band's edge, k is the tile's
    plane that coincides (in exact arithmetic) with the band's"""
    cols, rws = geo.group_rects(rows)
    out = []
    if axis == 0:
        for rect in cols:
            tx0, tx1 = rect[0] // TILE, rect[2] // TILE - 1
            for ty in range(rows[0], rows[1]):
                out += [((tx0, ty), 0, rect), ((tx1, ty), 1, rect)]
    else:
        for rect in rws + [geo.select_rect(rows)]:
            ty0, ty1 = rect[1] // TILE, rect[3] // TILE - 1
            for tx in range(geo.Tx):
                out += [((tx, ty0), 2, rect), ((tx, ty1), 3, rect)]
    return out


def band_edges(size, per_axis=44, total=768, seed=2) -> Case:
    """Lights outside a plane of a group column, a group row or a whole band (the rectangles of k0_lights and k0_band_count, for the whole frame and
    for the bands of 2 and 3 ranks), with r == -d_tile for a tile on that edge: the tile lists the light by a hair.  Of the candidates only those
    are kept whose distance from the BAND's plane (oracle_np.rect_frustum of the band's rectangle: other last bits than the tile's) is d_band < -r
    in fp32 -- exactly the lights a pre-filter without a margin drops."""
    cam = make_cam(size)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    depth = synth.make_linear_depth(size[0], size[1], seed)
    chosen = []
    quota = [(None, 0, per_axis), (None, 1, per_axis)] + [(r, 1, 12) for r in RANKS]
    for rank_of, axis, want in quota:
        edges = edge_tiles(geo, geo.band_rows(rank_of), axis)
        got, tries = 0, 0
        while got < want and tries < 40 * want:
            tries += 1
            tile, k, rect = edges[rng.integers(len(edges))]
            s_rel = (0.05 + 0.9 * rng.random()) if tries % 2 else (1.5 + 3.0 * rng.random())
            one = tangent_lights(geo, depth, [(tile, k, 0, s_rel)], rng)
            px, py, pz = oracle_np.view_positions(geo.fb, one)
            d_band = plane_d(geo.rect_planes(rect)[k], px[0], py[0], pz[0])
            if d_band < -one["bounds"][0, 0] and pz[0] - one["bounds"][0, 0] > 0:      # (... and only a sphere in front of the eye is ever dropped)
                chosen.append(one)
                got += 1
        assert got == want, (rank_of, axis, got)
    L = cat(chosen)
    lights = cat([L, filler(cam, depth, total - len(L), seed)])
    return Case(cam, depth, lights, {"band_hair_x": 32, "band_hair_y": 32, "band_hair_y_rank2": 1, "band_hair_y_rank3": 1, "select_hair": 1},
                constructed=len(L))


def margin_window(size, per=12, total=640, seed=3) -> Case:
    """Lights at d_band = -(r + k m), k in {0.5, 0.999, 1.001, 2}, m = 1e-3 (|x| + |y| + |z| + |r|): either side of the pre-filter's own threshold.
    No tile lists them (they lie k m outside a plane every tile of the band shares); the lists must not care on which side of the threshold."""
    cam = make_cam(size)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    depth = synth.make_linear_depth(size[0], size[1], seed)
    L = []
    for axis in (0, 1):
        edges = edge_tiles(geo, geo.band_rows(None), axis)
        for kk in (0.5, 0.999, 1.001, 2.0):
            for _ in range(per):
                tile, k, rect = edges[rng.integers(len(edges))]
                pv = outside_point(geo, depth, tile, k, rng, 0.3 + 2.0 * rng.random())
                one = blank_lights(1)
                one["worldPosition"][0] = geo.to_world(pv)
                px, py, pz = (v[0].astype(np.float64) for v in oracle_np.view_positions(geo.fb, one))
                s = -float(plane_d(geo.rect_planes(rect)[k].astype(np.float64), px, py, pz))
                a = abs(px) + abs(py) + abs(pz)
                r = (s - kk * 1e-3 * a) / (1.0 + kk * 1e-3)          # s = r + k m(r)
                assert r > 0
                set_radius(one, 0, r)
                L.append(one)
    L = cat(L)
    lights = cat([L, filler(cam, depth, total - len(L), seed)])
    return Case(cam, depth, lights, {"margin_inside": 2 * per, "margin_outside": 2 * per}, constructed=len(L))


# ---- eye_plane ----------------------------------------------------------------------------------------------------------------------------------
def eye_plane(size, total=640, seed=4) -> Case:
    """Spheres whose z - r straddles the margin m (the `inFront` switch: only a sphere entirely in front of the eye may be dropped by a side plane):
    z - r = k m for k in {-2, 0, 0.5, 0.999, 1.001, 2, 50}, laterally outside the frustum, over it, containing the eye, and behind the eye with a
    radius that reaches a tile."""
    cam = make_cam(size)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    depth = synth.make_linear_depth(size[0], size[1], seed)
    edge = abs(geo.ray(0.0, 0.0)[0])
    pts = []
    for kk in (-2.0, 0.0, 0.5, 0.999, 1.001, 2.0, 50.0):
        for lateral in (-6.0, -2.5, -1.05, -0.5, 0.0, 0.7, 1.2, 3.0, 8.0):       # x in units of the frustum's half-width at depth z
            for z in (0.5, 7.0, 120.0):
                x = lateral * edge * z
                y = (0.6 * rng.random() - 0.3) * z
                a = abs(x) + abs(y) + abs(z)
                r = (z - kk * 1e-3 * a) / (1.0 + kk * 1e-3)                        # z - r = k m(r)
                pts.append(((x, y, z), r))
    for _ in range(24):                                                            # containing the eye
        p = rng.normal(size=3) * 20.0
        pts.append(((p[0], p[1], p[2]), float(np.linalg.norm(p)) * (1.01 + rng.random())))
    for _ in range(24):                                                            # behind the eye, reaching a tile's depth range or not
        z = -(1.0 + 200.0 * rng.random())
        pts.append((((2 * rng.random() - 1) * 50.0, (2 * rng.random() - 1) * 50.0, z), -z + 3000.0 * rng.random() ** 3))
    L = blank_lights(len(pts))
    for j, (pv, r) in enumerate(pts):
        L["worldPosition"][j] = geo.to_world(pv)
        set_radius(L, j, r)
    lights = cat([L, filler(cam, depth, total - len(L), seed)])
    return Case(cam, depth, lights, {"eye_in_front_near": 16, "eye_not_in_front_near": 16, "eye_not_in_front_listed": 8, "eye_not_in_front_unlisted": 8,
                                     "eye_contains": 16, "eye_behind_listed": 4}, constructed=len(L))


# ---- depth_bounds -------------------------------------------------------------------------------------------------------------------------------
DEPTH_KINDS = ("flat", "two_level", "mixed_inf", "sky", "nan", "neg_zero", "negative", "denormal", "two_denormals", "noise")
RAW_KINDS = ("flat", "two_level", "mixed_inf", "sky", "denormal", "noise")


def depth_image(size, kinds, rng):
    """a depth image whose tiles cycle through `kinds` (tile t = ty Tx + tx gets kinds[t % len]); the special texel(s) of a tile sit at random valid
    pixels of it -- on the ragged border that is often a clamped row or column -- -> (image, kind index per tile)"""
    W, H = size
    Tx, Ty = (W - 1) // TILE + 1, (H - 1) // TILE + 1
    img = np.empty((H, W), F)
    kind = np.zeros((Ty, Tx), np.int64)
    for ty in range(Ty):
        for tx in range(Tx):
            k = kinds[(ty * Tx + tx) % len(kinds)]
            kind[ty, tx] = kinds.index(k)
            ys = np.arange(max(H - TILE * (ty + 1), 0), H - TILE * ty)           # tile row ty covers these framebuffer rows (row 0 = top)
            xs = np.arange(TILE * tx, min(TILE * (tx + 1), W))
            base = F(20.0 * 2.0 ** (5.0 * rng.random()))
            blk = np.full((len(ys), len(xs)), base, F)
            pick = lambda: (rng.integers(len(ys)), rng.integers(len(xs)))
            if k == "two_level":
                blk[pick()] = base * F(1.0 + rng.random())
                blk[pick()] = base * F(0.3 + 0.6 * rng.random())
            elif k == "mixed_inf":
                blk[rng.random(blk.shape) < 0.4] = np.inf
                blk[0, 0], blk[-1, -1] = base, np.inf
            elif k == "sky":
                blk[:] = np.inf
            elif k == "nan":
                blk[pick()] = np.nan
            elif k == "neg_zero":
                blk[pick()] = -0.0
            elif k == "negative":
                blk[pick()] = -F(1.0 + 50.0 * rng.random())
            elif k == "denormal":
                blk[pick()] = F(1e-41)
            elif k == "two_denormals":
                blk[:] = F(3e-41)
                blk[pick()] = F(1e-41)
            elif k == "noise":
                blk[:] = (base * (0.5 + rng.random(blk.shape))).astype(F)
            img[np.ix_(ys, xs)] = blk
    return img, kind


def depth_bounds(size, raw=False, total=640, seed=5) -> Case:
    """For every tile whose swapped bounds (z_far' = z_far - diff, z_near' = z_near + diff: inexact in fp32, the rounded values count) are finite:
    spheres on the tile's centre ray with fl(pz - r) equal to z_near', the float above (rejected) and the float below, and fl(pz + r) equal to
    z_far', above and below (rejected).  raw: the image is a reversed-Z attachment (0 = nothing drawn) and `depth` its linearisation."""
    cam = make_cam(size)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    if raw:
        lin, _ = depth_image(size, RAW_KINDS, rng)
        with np.errstate(divide="ignore", over="ignore"):
            raw_img = np.where(np.isinf(lin), F(0.0), np.where(lin < 1e-30, F(1e-41), F(cam.z_near) / lin)).astype(F)
        depth = oracle.linearize_depth(cam.z_near, raw_img)
    else:
        raw_img = None
        depth, _ = depth_image(size, DEPTH_KINDS, rng)
    L = []
    for ty in range(geo.Ty):
        for tx in range(geo.Tx):
            bits = geo.tile_depth(depth, tx, ty).view(np.uint32)
            with np.errstate(invalid="ignore"):
                z_far, z_near = bits.max().view(F), bits.min().view(F)
                diff = z_far - z_near
                z_far, z_near = z_far - diff, z_near + diff
            if not (np.isfinite(z_far) and np.isfinite(z_near)):
                z_far = z_near = None
            ray = geo.ray(tx * TILE + 8.0, ty * TILE + 8.0)
            for which, bound in (("near", z_near), ("far", z_far)):
                for c in (0, 1, -1):
                    one = blank_lights(1)
                    if bound is None:              # no finite bound to touch: a sphere that only the depth test could reject
                        pz, r = F(10.0 ** rng.uniform(0, 4)), F(0.25)
                    else:
                        r = F(max(abs(float(bound)), 1e-3) * (0.05 + 0.2 * rng.random()))
                        if which == "near" and bound <= 0:                       # (a sign-bit texel: the bound is negative or zero)
                            r = F((abs(float(bound)) + 1.0) * (1.5 + rng.random()))
                        if bound != 0 and abs(bound) < np.finfo(F).tiny:          # a denormal bound: a point light ON it, r = 0
                            r = F(0.0)
                        start = F(bound + r) if which == "near" else F(bound - r)
                        pz = None
                        for step in range(-4, 5):
                            cand = up(start, step) if step >= 0 else down(start, -step)
                            op = F(cand - r) if which == "near" else F(cand + r)
                            if ordinal(op) - ordinal(bound) == c:
                                pz = cand
                                break
                        if pz is None or not pz > 0:
                            continue
                    one["worldPosition"][0] = geo.to_world(ray * float(pz))
                    set_radius(one, 0, r)
                    vz = oracle_np.view_positions(geo.fb, one)[2][0]
                    if vz != pz:                   # (the view transform is exact for this camera; were it not, the light would not be on its float)
                        continue
                    L.append(one)
    L = cat(L)
    n_fill = max(total - len(L), 64)
    fill = blank_lights(n_fill)                    # filler at all depths over the whole frame: the depth test decides most of them
    for j in range(n_fill):
        z = 10.0 ** rng.uniform(0.5, 3.3)
        fill["worldPosition"][j] = geo.to_world(geo.ray(rng.uniform(0, size[0]), rng.uniform(0, size[1])) * z)
        set_radius(fill, j, z * rng.uniform(0.01, 0.4))
    lights = cat([L, fill])
    names = ["depth_near_eq", "depth_near_above", "depth_near_below", "depth_far_eq", "depth_far_above", "depth_far_below"]
    expect = {n: 8 for n in names}
    expect.update({"tiles_flat": 1, "tiles_mixed_inf": 1, "tiles_sky": 1})
    if not raw:
        expect.update({"tiles_nan": 1, "tiles_sign_bit": 2, "tiles_denormal": 1})
    return Case(cam, depth, lights, expect, raw_depth=raw_img, constructed=len(L))


# ---- degenerate_lights --------------------------------------------------------------------------------------------------------------------------
def degenerate_lights(size, total=640, seed=6, view="affine") -> Case:
    """Records no sane scene holds: NaN and +-inf position components, radius 0 / negative / +inf / NaN / denormal, positions with denormal components
    (beside the screen's vertical centre line the tile plane is x = 0 to the last bit, so d is the denormal px itself and `d < -r` is decided between
    two denormals: flushing either to zero flips it), coordinates near 1e30 (the dot product overflows)."""
    cam = make_cam(size, view=view)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    depth = synth.make_linear_depth(size[0], size[1], seed)
    base = filler(cam, depth, 160, seed + 1)
    L = base.copy()
    pos, rad = L["worldPosition"], L["bounds"]
    specials = [np.nan, np.inf, -np.inf]
    for j in range(0, 36):                                        # one non-finite position component
        pos[j, j % 3] = specials[(j // 3) % 3]
    for j, r in zip(range(36, 76), [0.0, -0.0, -1.0, -1e-3, -1e30, np.inf, -np.inf, np.nan, 1e-41, -1e-41] * 4):
        rad[j] = F(r)
    for j in range(76, 116):                                      # denormal positions, denormal radii: on and beside the eye's axis
        d = lambda: F((rng.integers(1, 4000) * 1e-42) * (1 if rng.random() < 0.5 else -1))
        pos[j] = geo.to_world((0.0, 0.0, 0.0))
        pos[j, 0] = d()
        pos[j, 2] = -abs(d()) if j % 2 else d()
        if j % 4 == 0:
            pos[j, 2] = -F(10.0 ** rng.uniform(-3, 3))            # denormal x at an ordinary depth
        rad[j] = F(rng.integers(0, 3000) * 1e-42) if j % 3 else F(10.0 ** rng.uniform(-3, 3))
    for j in range(116, 160):                                     # coordinates near 1e30
        p = rng.normal(size=3) * 1e30                                 # (the impact's squares overflow)
        if j % 4 >= 2:                                                # (... and near FLT_MAX the plane distance itself: +-inf, or inf - inf)
            p = rng.uniform(2.5e38, 3.3e38, 3) * rng.choice([-1.0, 1.0], 3)
        p[2] = -abs(p[2]) if j % 2 else p[2]
        pos[j] = p.astype(F)
        rad[j] = F(10.0 ** rng.uniform(-2, 31)) if j % 3 else F(3e38)
    lights = cat([L, filler(cam, depth, total - len(L), seed)])
    return Case(cam, depth, lights, {"nan_position": 8, "inf_position": 16, "radius_zero": 4, "radius_negative": 8, "radius_inf": 4, "radius_nan": 4,
                                     "radius_denormal": 4, "position_denormal": 16, "denormal_decides": 1, "dot_overflow": 8}, constructed=160)


# ---- ties_and_counts ----------------------------------------------------------------------------------------------------------------------------
GROUP_AT = (1, 0)            # the group the counted lights sit in: tile columns 4 .. 7, tile rows 0 .. 3 -- a group of its own on the whole frame and on
                             # the first band of 2 and of 3 ranks (whose rows 0 .. 5 resp. 0 .. 3 start at tile row 0)
GLOBALS = 3                  # lights every tile lists: two directional ones and a sphere so large and far that its impact is +inf


def counts(size, group_total, tile_counts=(128, 129, 196, 197), others=96, seed=7, expect=None) -> Case:
    """Exactly `group_total` candidates in the 4 x 4-tile group GROUP_AT and nothing doubtful anywhere: the GLOBALS, then small spheres deep inside
    single tiles of the group (a tenth of a tile wide, around the tile's centre ray at the tile's flat depth), `tile_counts[i]` of everything
    for tile i of the group and the rest over its other tiles; `others` more of the same in a group far away.  A counted tile's lights hold the ties:
    duplicate records, pairs mirrored about the tile's centre (pz - cz = +-2^-k exactly), the directional 0s and the +inf impact."""
    cam = make_cam(size)
    geo = Geo(cam)
    rng = np.random.default_rng(seed)
    W, H = size
    depth = np.full((H, W), F(64.0))
    glob = blank_lights(GLOBALS)
    glob["type"][:2] = host.LIGHT_DIRECTIONAL
    glob["worldPosition"][2] = geo.to_world((1e25, 0.0, 1e3))
    set_radius(glob, 2, 3e25)
    gx, gy = GROUP_AT
    group_tiles = [(gx * GROUP + i % GROUP, gy * GROUP + i // GROUP) for i in range(GROUP * GROUP)]
    local = group_total - GLOBALS
    per_tile = [c - GLOBALS for c in tile_counts]
    rest = local - sum(per_tile)
    assert rest >= 0
    spare = len(group_tiles) - len(per_tile)
    per_tile += [rest // spare + (1 if i < rest % spare else 0) for i in range(spare)]
    z = 64.0

    def inside(tile, n, ties):
        centre = geo.ray(tile[0] * TILE + 8.0, tile[1] * TILE + 8.0) * z
        out = blank_lights(n)
        width = abs(geo.ray(TILE, 0)[0] - geo.ray(0, 0)[0]) * z
        for j in range(n):
            pv = centre + np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 0.0]) * width + np.array([0, 0, rng.uniform(-0.5, 0.5) * 0.05 * width])
            if ties and j % 4 == 1:                      # mirrored about the tile's centre in z (cz = 64 exactly: the depth is flat): pz - cz = +-2^-k, the
                k = 2.0 ** -(2 + (j // 8) % 3)           # same x and y -- the same impact as its partner, to the bit
                pv = np.array([centre[0], centre[1], z + k if j % 8 == 1 else z - k])
            out["worldPosition"][j] = geo.to_world(pv)
            set_radius(out, j, 0.05 * width)
            if ties and j % 4 == 3 and j > 0:            # a duplicate record
                out[j] = out[j - 1]
        return out

    parts = [glob]
    for i, (tile, n) in enumerate(zip(group_tiles, per_tile)):
        parts.append(inside(tile, n, ties=i < len(tile_counts)))
    far_tiles = [(geo.Tx - 2, geo.Ty - 2), (geo.Tx - 3, geo.Ty - 2)]
    for i in range(others):
        parts.append(inside(far_tiles[i % 2], 1, False))
    lights = cat(parts)
    exp = {f"tiles_{c}": 1 for c in tile_counts}
    exp.update({"tie_tiles": 1, "inf_impact_tiles": 1, "directional_in_selection": 1})
    exp.update(expect or {})
    return Case(cam, depth, lights, exp, constructed=len(lights), notes={"group_max": group_total})


# ---- wide_forms ---------------------------------------------------------------------------------------------------------------------------------
def wide(size, total, per=3, seed=8, fov=90.0, expect=None) -> Case:
    """the tangent lights of `tile_planes` first, then a few ordinary lights, then cheap filler far outside the frustum up to `total`"""
    c = tile_planes(size, per=per, total=12 * per + 200, fov=fov, seed=seed)
    geo = Geo(c.cam)
    rng = np.random.default_rng(seed)
    lights = cat([c.lights, far_filler(geo, total - len(c.lights), rng)])
    return Case(c.cam, c.depth, lights, expect if expect is not None else {f"plane{k}_{n}": 1 for k in range(4) for n in ("eq", "above", "below")},
                constructed=c.constructed)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
NARROW = fov_for(9.0e3)                       # p11 = 9.0e3 (p00 = p11 / aspect): just inside the `sane` gate's upper end
TOO_NARROW = fov_for(1.4e4, 1.0)              # p11 = 1.4e4 > 1e4: the brute-force walk
LOOSE = {k: 1 for k in PLANE_EXPECT}          # (small sets: every plane and radius class still occurs)

CASES = {
    "tile_planes":            lambda: tile_planes(BIG),
    "tile_planes-ragged":     lambda: tile_planes(RAGGED, seed=11),
    "tile_planes-scaled":     lambda: tile_planes(RAGGED, view="scaled", seed=12),
    "band_edges":             lambda: band_edges(BIG),
    "band_edges-ragged":      lambda: band_edges(RAGGED, per_axis=36, seed=13),
    "margin_window":          lambda: margin_window(BIG),
    "eye_plane":              lambda: eye_plane(BIG),
    "depth_bounds":           lambda: depth_bounds(BIG),
    "depth_bounds-ragged":    lambda: depth_bounds(RAGGED, seed=14),
    "depth_bounds-raw":       lambda: depth_bounds(RAGGED, raw=True, seed=15),
    "degenerate":             lambda: degenerate_lights(BIG),
    "degenerate-scaled":      lambda: degenerate_lights(RAGGED, view="scaled", seed=16),
    # exactly this many candidates in one group (HEAVY_MIN_BAND, HEAVY_MIN_FRAME, CAPG and one more), the counted tiles inside it
    "counts-384":             lambda: counts(BIG, 384, tile_counts=(128, 129), others=160),
    "counts-385":             lambda: counts(BIG, 385, tile_counts=(196, 129), others=160),
    "counts-512":             lambda: counts(BIG, 512, tile_counts=(128, 197), others=32),
    "counts-513":             lambda: counts(BIG, 513, tile_counts=(196, 197), others=32),
    "counts-2048":            lambda: counts(BIG, 2048),
    "counts-2049":            lambda: counts(BIG, 2049),
    # light counts either side of the brute-force threshold and of a mask word / a 64-light block
    **{f"n-{n}": (lambda n=n: tile_planes(RAGGED, per=6, total=n, seed=20 + n % 7, expect=LOOSE)) for n in (511, 512, 513, 575, 576, 577)},
    # fields of view at the ends of the `sane` gate (light_cull.hip: p00, p11 in (1e-2, 1e4)); outside it the entry point takes the brute-force walk
    "perspective-wide":       lambda: tile_planes(BIG, fov=fov_for(1.02e-2, 256 / 192), seed=31),
    "perspective-narrow":     lambda: tile_planes(BIG, fov=NARROW, seed=32),
    "perspective-too_wide":   lambda: tile_planes(RAGGED, per=6, total=600, fov=fov_for(0.98e-2, 131 / 77), seed=33, expect=LOOSE),
    "perspective-too_narrow": lambda: tile_planes(RAGGED, per=6, total=600, fov=TOO_NARROW, seed=34, expect=LOOSE),
    # the large-set kernels on tiny frames
    # 65 group columns: the second 64-band window of the interval masks holds one band (aspect 130: at 90 degrees p00 = 1 / 130 would fail the `sane` gate
    # and the frame take the brute-force walk -- p00 = 0.05, p11 = 6.5 here)
    "wide-65_columns":        lambda: wide((4160, 32), 1200, per=8, fov=fov_for(0.05, 130.0)),
    "wide-27_bands":          lambda: wide((1088, 640), 640, per=4),          # 17 + 10 bands > 24: the plane-test form splits them over two blocks
    "wide-4096_words":        lambda: wide((64, 64), 262144),                 # k1_group_lists_wide<EXACT>
    "wide-4098_words":        lambda: wide((64, 64), 262272),                 # ... the bounds-checked one
}
BRUTE = {"n-511", "perspective-too_wide", "perspective-too_narrow"}           # cases whose default path IS the brute-force walk
HUGE = {"wide-4096_words", "wide-4098_words"}


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    return CASES[name]()


# ---- references, computed once per case ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c_lists(name: str, rank_of=None):
    """the C oracle's (grid, indices, counts) of the whole frame or of a band"""
    c = build(name)
    W, H = c.size
    rows = None if rank_of is None else Geo(c.cam).band_rows(rank_of)
    return oracle.light_cull(c.cam.frame, W, H, c.lights, c.depth, tile_rows=rows, want_counts=True, threads=min(8, oracle.host_threads()))


def table_lights(c: Case):
    """the lights the tables are taken over: all of them, but for the huge sets the constructed and ordinary ones in front (the far filler behind them
    is rejected by every tile: the C oracle's lists say so)"""
    return c.lights if len(c.lights) <= 8192 else c.lights[: c.constructed + 200]


@functools.lru_cache(maxsize=None)
def tables(name: str):
    c = build(name)
    W, H = c.size
    fb = bytes(c.cam.frame)
    L = table_lights(c)
    ok32, _, ops = oracle_np.overlap_table(fb, W, H, L, c.depth, np.float32, want_operands=True)
    ok64, slack = oracle_np.overlap_table(fb, W, H, L, c.depth, np.float64)
    return ok32, ops, ok64, slack


def finite_lights(ops) -> np.ndarray:
    """bool[N]: every operand of every comparison of the light is finite (the tile bounds aside)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(ops["near"]) & np.isfinite(ops["far"]) & np.isfinite(ops["neg_r"]) & np.isfinite(ops["d"]).all(axis=(0, 2))


def band_keep(c: Case, rows, margin, L=None):
    """light_cull.hip's pre-filter restated in fp32 for the band of tile rows `rows`: (keep_col bool[groupsX, N], keep_row bool[groupsY, N],
    keep_select bool[N]) -- a light stays in a band's mask unless it lies entirely in front of the eye (z - r > m) and beyond one of the band's
    two planes by more than m = margin (|x| + |y| + |z| + |r|); directional lights always stay.  margin = 0: the pre-filter without its margin."""
    geo = Geo(c.cam)
    L = table_lights(c) if L is None else L
    px, py, pz = oracle_np.view_positions(geo.fb, L)
    r = L["bounds"][:, 0].astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        m = F(margin) * ((np.abs(px) + np.abs(py)) + (np.abs(pz) + np.abs(r)))
        in_front = (pz - r) > m
        thr = -(r + m)
        always = (L["type"] == 0) | ~in_front
        cols, rws = geo.group_rects(rows)

        def keep(rect, a, b):
            pl = geo.rect_planes(rect)
            return always | ~((plane_d(pl[a], px, py, pz) < thr) | (plane_d(pl[b], px, py, pz) < thr))
        stack = lambda rows_: np.stack(rows_) if rows_ else np.zeros((0, len(L)), bool)
        return (stack([keep(rc, 0, 1) for rc in cols]), stack([keep(rc, 2, 3) for rc in rws]), keep(geo.select_rect(rows), 2, 3),
                dict(m=m, in_front=in_front, thr=thr))


def dropped_though_listed(c: Case, ok32, rows, margin):
    """-> (lights a tile of the band lists (fp32 table) although the pre-filter with `margin` drops them from the tile's group column, ... group row,
    ... from the band's selection): bool[N] each"""
    geo = Geo(c.cam)
    kc, kr, ks, _ = band_keep(c, rows, margin)
    r0, r1 = rows
    N = ok32.shape[1]
    x, y, s = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    for ty in range(r0, r1):
        for tx in range(geo.Tx):
            row = ok32[ty * geo.Tx + tx]
            x |= row & ~kc[tx // GROUP]
            y |= row & ~kr[(ty - r0) // GROUP]
            s |= row & ~ks
    return x, y, s


def coverage(name: str) -> dict:
    """what the case reaches, counted on the tables: see the families' docstrings for the names"""
    c = build(name)
    geo = Geo(c.cam)
    ok32, ops, ok64, slack = tables(name)
    L = table_lights(c)
    T, N = ok32.shape
    cov = {"n_lights": len(c.lights), "pairs": int(ok32.size)}
    fin = finite_lights(ops)
    cov["fp32_ne_fp64"] = int((ok32 != ok64)[:, fin].sum())
    cov["slack_below_1e-6"] = int((slack[:, fin] < 1e-6).sum())
    # each comparison's verdict, and the pairs whose five OTHER comparisons accept: there the one comparison decides
    point = (L["type"] != 0)[None, :]
    with np.errstate(invalid="ignore"):
        rej = np.concatenate([(ops["near"][None, :] > ops["z_near"][:, None])[..., None], (ops["far"][None, :] < ops["z_far"][:, None])[..., None],
                              ops["d"] < ops["neg_r"][None, :, None]], axis=2)                      # [T, N, 6]
    others_accept = (rej.sum(2)[..., None] - rej) == 0
    cls = {"eq": 0, "above": 1, "below": -1}
    for k in range(4):
        dist = ordinal(ops["d"][..., k]) - ordinal(ops["neg_r"])[None, :]
        usable = np.isfinite(ops["d"][..., k]) & point & others_accept[..., 2 + k]
        for nme, v in cls.items():
            cov[f"plane{k}_{nme}"] = int(((dist == v) & usable).sum())
    for i, (which, bound) in enumerate((("near", "z_near"), ("far", "z_far"))):
        dist = ordinal(ops[which])[None, :] - ordinal(ops[bound])[:, None]
        usable = np.isfinite(ops[which])[None, :] & np.isfinite(ops[bound])[:, None] & point & others_accept[..., i]
        for nme, v in cls.items():
            cov[f"depth_{which}_{nme}"] = int(((dist == v) & usable).sum())
    # the tiles' depth content
    kinds = {"tiles_flat": 0, "tiles_mixed_inf": 0, "tiles_sky": 0, "tiles_nan": 0, "tiles_sign_bit": 0, "tiles_denormal": 0}
    for ty in range(geo.Ty):
        for tx in range(geo.Tx):
            td = geo.tile_depth(c.depth, tx, ty)
            b = td.view(np.uint32)
            kinds["tiles_flat"] += int(b.min() == b.max() and np.isfinite(td).all())
            kinds["tiles_mixed_inf"] += int(np.isinf(td).any() and np.isfinite(td).any())
            kinds["tiles_sky"] += int(np.isposinf(td).all())
            kinds["tiles_nan"] += int(np.isnan(td).any())
            kinds["tiles_sign_bit"] += int((b >> 31).any())
            kinds["tiles_denormal"] += int(((td != 0) & (np.abs(td) < np.finfo(F).tiny)).any())
    cov.update(kinds)
    # the pre-filter: what it would drop without its margin, and what it drops with it (nothing, or the kernel's argument is wrong)
    x0, y0, _ = dropped_though_listed(c, ok32, (0, geo.Ty), 0.0)
    cov["band_hair_x"], cov["band_hair_y"] = int(x0.sum()), int(y0.sum())
    sel = np.zeros(N, bool)
    margin_drops = 0
    for world in (2, 3):
        yy = np.zeros(N, bool)
        for rank in range(world):
            rows = geo.band_rows((rank, world))
            _, y, s = dropped_though_listed(c, ok32, rows, 0.0)
            yy |= y
            sel |= s
            margin_drops += sum(int(v.sum()) for v in dropped_though_listed(c, ok32, rows, MARGIN))
        cov[f"band_hair_y_rank{world}"] = int(yy.sum())
    cov["select_hair"] = int(sel.sum())
    cov["margin_drops"] = margin_drops + sum(int(v.sum()) for v in dropped_though_listed(c, ok32, (0, geo.Ty), MARGIN))
    # either side of the kernel's own threshold: k = (-d_band - r) / m of the nearest band plane that has the light outside it
    kc, kr, _, aux = band_keep(c, (0, geo.Ty), MARGIN)
    px, py, pz = ops["px"], ops["py"], ops["pz"]
    r = -ops["neg_r"]
    cols, rws = geo.group_rects((0, geo.Ty))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        kmin = np.full(N, np.inf)
        for rects, pair in ((cols, (0, 1)), (rws, (2, 3))):
            for rect in rects:
                for a in pair:
                    k = (-plane_d(geo.rect_planes(rect)[a], px, py, pz).astype(np.float64) - r) / aux["m"]
                    kmin = np.where((k > 0) & (k < kmin), k, kmin)
        ok_pt = aux["in_front"] & (L["type"] != 0)
        cov["margin_inside"] = int((ok_pt & (kmin > 0.2) & (kmin < 1.0)).sum())
        cov["margin_outside"] = int((ok_pt & (kmin > 1.0) & (kmin < 3.0)).sum())
        # the inFront switch
        zr = (pz - r).astype(np.float64) / aux["m"]
        listed = ok32.any(0)
        pt = L["type"] != 0
        cov["eye_in_front_near"] = int((pt & aux["in_front"] & (zr < 3.0)).sum())
        cov["eye_not_in_front_near"] = int((pt & ~aux["in_front"] & (zr > -3.0)).sum())
        cov["eye_not_in_front_listed"] = int((pt & ~aux["in_front"] & listed & np.isfinite(zr)).sum())
        cov["eye_not_in_front_unlisted"] = int((pt & ~aux["in_front"] & ~listed & np.isfinite(zr)).sum())
        cov["eye_contains"] = int((pt & (r > np.sqrt(px.astype(np.float64) ** 2 + py.astype(np.float64) ** 2 + pz.astype(np.float64) ** 2))).sum())
        cov["eye_behind_listed"] = int((pt & (pz < 0) & listed).sum())
        # records no sane scene holds
        wp, rad = L["worldPosition"], L["bounds"][:, 0]
        tiny = np.finfo(F).tiny
        cov["nan_position"] = int(np.isnan(wp).any(1).sum())
        cov["inf_position"] = int(np.isinf(wp).any(1).sum())
        cov["radius_zero"] = int((rad == 0).sum())
        cov["radius_negative"] = int((rad < 0).sum())
        cov["radius_inf"] = int(np.isinf(rad).sum())
        cov["radius_nan"] = int(np.isnan(rad).sum())
        cov["radius_denormal"] = int(((rad != 0) & (np.abs(rad) < tiny)).sum())
        cov["position_denormal"] = int(((wp != 0) & (np.abs(wp) < tiny)).any(1).sum())
        den = lambda a: (a != 0) & (np.abs(a) < tiny)
        cov["denormal_decides"] = int((den(ops["d"]) & den(ops["neg_r"])[None, :, None] & (ops["d"] < ops["neg_r"][None, :, None])).sum())
        cov["dot_overflow"] = int((np.isfinite(wp).all(1) & ~np.isfinite(ops["d"]).all(axis=(0, 2))).sum())
    # list lengths, ties among the impacts of a tile whose selection runs
    cnt = ok32.sum(1)
    for n in (128, 129, 196, 197):
        cov[f"tiles_{n}"] = int((cnt == n).sum())
    cov["tiles_over_196"] = int((cnt > CAND).sum())
    cov["tiles_over_128"] = int((cnt > KEEP).sum())
    tie = inf_imp = dir_sel = 0
    for t in np.nonzero(cnt > KEEP)[0]:
        tx, ty = int(t) % geo.Tx, int(t) // geo.Tx
        cand = np.nonzero(ok32[t])[0][:CAND]
        _, cx, cy = oracle_np.tile_frustum(geo.inv, tx, ty, geo.vp_w, geo.vp_h)
        with np.errstate(invalid="ignore", over="ignore"):
            cz = (ops["z_far"][t] + ops["z_near"][t]) * F(0.5)
            dx, dy, dz = px[cand] - cx, py[cand] - cy, pz[cand] - cz
            imp = np.sqrt((dx * dx + dy * dy) + dz * dz).astype(F)
        imp[L["type"][cand] == 0] = F(0.0)
        finite = imp[np.isfinite(imp) & (imp > 0)]
        tie += int(len(np.unique(finite)) < len(finite))
        inf_imp += int(np.isposinf(imp).any())
        dir_sel += int((L["type"][cand] == 0).any())
    cov["tie_tiles"], cov["inf_impact_tiles"], cov["directional_in_selection"] = tie, inf_imp, dir_sel
    # the group lists: (column mask) AND (row mask), per band configuration
    for label, rank_of in (("frame", None), ("rank0of2", (0, 2)), ("rank0of3", (0, 3))):
        rows = geo.band_rows(rank_of)
        kc, kr, _, _ = band_keep(c, rows, MARGIN, c.lights if len(c.lights) <= 8192 else None)
        per_group = (kc[None, :, :] & kr[:, None, :]).sum(2)
        cov[f"group_max_{label}"] = int(per_group[per_group <= CAPG].max()) if (per_group <= CAPG).any() else 0   # (as cull_diagnostics counts it)
        cov[f"groups_over_capg_{label}"] = int((per_group > CAPG).sum())
    return cov
