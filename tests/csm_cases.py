"""Small scenes for the directional shadow term (Standard.shader:266-283, Lighting.glsl:168-284), shared by tests/test_csm_cpu.py (C oracle against
the float64 restatement) and tests/test_csm_gpu.py (the kernels against both).  Frames are 96 x 64 or 40 x 24 (a ragged last tile column), maps at most
64 texels a side, light 0 is directional with the case's shadowType; a wave of the shade kernels is an 8 x 8-pixel quadrant (both heights are
multiples of 8, so quadrant (y // 8, x // 8) of the framebuffer is one wave).

Two families:

  scene   the synthetic camera, a depth field, sailor_amd.host.csm_matrices' four matrices (or a projective variant of them) and maps whose values
          are centred on the fragments' own light-space depth, so that the compares fall both ways inside a quadrant
  direct  light matrices that are a pure scale and offset of world x, y, z (powers of two: every product and sum of the chain is exact in fp32), and
          world positions computed back from the light-space coordinates a pixel is meant to have: px, py land exactly on 0, 1, the floats beside
          them, texel centres and texel borders; pz on the look-up's limit and beside it; the cascade is chosen by |world z|

The camera sits at (0, 150, 0) with the identity rotation: the view matrix is a translation along y, a fragment's view depth IS -world z, exactly."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle
from sailor_amd import host, synth

BIG, SMALL = (96, 64), (40, 24)
Z_FAR = 20000.0
THRESHOLDS = (np.float32(Z_FAR) * np.asarray([0.05, 0.1, 0.333333, 0.5], np.float32)).astype(np.float32)   # RN(zFar * level[i]): one fp32 product
MID_DEPTH = np.array([500.0, 1500.0, 4000.0, 9000.0])                                                       # a depth well inside each cascade


@dataclass
class Case:
    frame: synth.Frame
    boundary: np.ndarray                      # bool[H, W]: pixels placed ON a cascade threshold or a rejection limit, or one float beside it
    expect: tuple = ()                        # names of the coverage counts (coverage()) that must be non-zero: what the case exists to reach
    notes: dict = field(default_factory=dict)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------------------
def light_rotation(yaw_deg: float, pitch_deg: float) -> np.ndarray:
    """unit quaternion (x, y, z, w): yaw about +Y, then pitch about +X (synth.directional_rotation is (25, -50))"""
    yaw, pitch = np.radians(yaw_deg), np.radians(pitch_deg)
    ax, ay, az, aw = 0.0, np.sin(yaw / 2), 0.0, np.cos(yaw / 2)
    bx, by, bz, bw = np.sin(pitch / 2), 0.0, 0.0, np.cos(pitch / 2)
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
    return (q / np.linalg.norm(q)).astype(np.float32)


def csm_matrices(cam, q) -> np.ndarray:
    light_view = host.mat4_inverse(host.transform_matrix([0, 0, 0, 0], q, [1, 1, 1, 1]))
    return host.csm_matrices(light_view, cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)


def projective(lm: np.ndarray, cascades) -> np.ndarray:
    """w row += 0.25 x row + 0.125 z row of the named cascades: w = 1 + 0.25 x + 0.125 z varies across the frame, is never exactly 1 and stays
    positive wherever x > -3 (checked on the case's own pixels in scene())"""
    out = lm.copy().reshape(4, 4, 4)          # [cascade, column, row]
    for c in cascades:
        out[c, :, 3] += np.float32(0.25) * out[c, :, 0] + np.float32(0.125) * out[c, :, 2]
    return out.reshape(4, 16)


def scaled_view(cam):
    """the camera with all sixteen entries of frame.view doubled: p.z / p.w is unchanged and w == 2 in every lane"""
    f = host.fill_frame_data(cam.world, cam.fov, cam.z_near, cam.z_far, cam.width, cam.height)
    for i in range(16):
        f.view[i] = f.view[i] * 2.0
    return synth.Camera(world=cam.world, fov=cam.fov, z_near=cam.z_near, z_far=cam.z_far, width=cam.width, height=cam.height, frame=f)


def directional_light(direction, shadow_type, extra: np.ndarray | None = None) -> np.ndarray:
    n = 1 + (0 if extra is None else len(extra))
    L = np.zeros(n, host.LIGHT_DTYPE)
    if extra is not None:
        L[1:] = extra
    L["type"][0] = host.LIGHT_DIRECTIONAL
    L["shadowType"][0] = shadow_type
    L["direction"][0] = np.asarray(direction, np.float32)
    L["intensity"][0] = np.float32([17.0, 13.0, 9.0])
    return L


def make_surface(cam, pos: np.ndarray, rng, lights) -> np.ndarray:
    """float32[3, H, W, 4] around the given world positions: normals tilted off the view direction as synth.make_surface's are, roughness U[0.3, 1],
    albedo U[0.05, 1]^3, metallic 0 or U[0, 1].  A pixel within reach of a directional light's specular peak (NdfGGX's denominator below 1e-2, where
    the rounding of cosLh is amplified by its reciprocal: what tests/test_oracle_cpu.py lists as the K2 bound's one exception) gets roughness 1."""
    H, W = pos.shape[:2]
    s = np.empty((3, H, W, 4), np.float32)
    s[0, ..., :3] = pos
    s[0, ..., 3] = 0.5 + 0.5 * rng.random((H, W))
    v = pos.astype(np.float64) - cam.world.reshape(4, 4)[3, :3].astype(np.float64)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    n = -v + 0.8 * (2.0 * rng.random((H, W, 3)) - 1.0)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    s[1, ..., :3] = n
    s[1, ..., 3] = 0.3 + 0.7 * rng.random((H, W))
    s[2, ..., :3] = 0.05 + 0.95 * rng.random((H, W, 3))
    s[2, ..., 3] = np.where(rng.random((H, W)) < 0.8, 0.0, rng.random((H, W)))
    n64 = s[1, ..., :3].astype(np.float64)
    for l in lights[lights["type"] == host.LIGHT_DIRECTIONAL]:
        lh = -l["direction"].astype(np.float64) - v
        lh /= np.linalg.norm(lh, axis=-1, keepdims=True)
        cl = np.maximum(0.0, (n64 * lh).sum(-1))
        a2 = s[1, ..., 3].astype(np.float64) ** 4
        s[1, ..., 3] = np.where(cl * cl * (a2 - 1.0) + 1.0 < 1e-2, np.float32(1.0), s[1, ..., 3])
    return np.ascontiguousarray(s)


def positions_at_depth(cam, depth: np.ndarray, sign: np.ndarray | None = None) -> np.ndarray:
    """the world position of every pixel's ray at view depth `depth` (world z = -depth exactly; sign = +1 puts it behind the camera at +depth)"""
    rx, ry = synth.pixel_rays(cam)
    d = depth.astype(np.float32)
    pos = np.stack([rx[None, :] * d, ry[:, None] * d + np.float32(150.0), -d], -1).astype(np.float32)
    if sign is not None:
        pos[..., 2] = np.where(sign > 0, d, -d)
    return pos


def quadrants(W: int, H: int) -> np.ndarray:
    """int[H, W]: the number of the pixel's 8 x 8 quadrant, row-major"""
    return (np.arange(H)[:, None] // 8) * ((W + 7) // 8) + np.arange(W)[None, :] // 8


# ---- depth fields of the cascade select -----------------------------------------------------------------------------------------------------------
def depth_ramp(W, H, rng):
    ramp = 60.0 * 300.0 ** ((np.arange(W) + 0.5) / W)                                    # 60 .. 18 000 across the frame: every cascade
    return (ramp[None, :] * (0.8 + 0.4 * rng.random((H, W)))).astype(np.float32), None, np.zeros((H, W), bool)


def depth_checker(W, H, rng, left_uniform=False):
    """pixels alternating between two cascades inside every quadrant, pairs (0, 1), (1, 2), (2, 3) by quadrant; left_uniform: the left half of the
    frame one cascade per quadrant instead (`mixed`: both dispatch paths in one launch)"""
    q = quadrants(W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    pair = q % 3
    c = pair + ((xs + ys) & 1)
    if left_uniform:
        c = np.where(xs < W // 2, q % 4, c)
    return (MID_DEPTH[c] * (0.9 + 0.2 * rng.random((H, W)))).astype(np.float32), None, np.zeros((H, W), bool)


def depth_boundaries(W, H, rng):
    """a quadrant each for: the fp32 view depth exactly RN(zFar * level[i]), the float below and the float above (i = 0..3), depths beyond
    zFar / 2 (cascade 4, clamped to 3), each at negative and at positive view z; the other quadrants keep the ramp"""
    depth, _s, _b = depth_ramp(W, H, rng)
    vals = []
    for t in THRESHOLDS:
        vals += [np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(np.inf))]
    vals += [np.float32(12000.0), np.float32(19000.0), np.float32(25000.0)]
    q = quadrants(W, H)
    sign = -np.ones((H, W))
    boundary = np.zeros((H, W), bool)
    assert q.max() + 1 >= 2 * len(vals)
    for k, v in enumerate(vals + vals):
        m = q == k
        depth[m] = v
        sign[m] = -1.0 if k < len(vals) else 1.0
        boundary |= m & (k % len(vals) < 12)
    return depth, sign, boundary


# ---- maps -----------------------------------------------------------------------------------------------------------------------------------------
def noise(rng, shape, lo, hi, dtype=np.float32):
    return (lo + (hi - lo) * rng.random(shape)).astype(dtype)


def evsm_moments(depth: np.ndarray, radii=None) -> np.ndarray:
    """ShadowCaster's moments of a depth image, blurred by ShadowPrepassNode's two passes (the C oracle's, which tests/test_oracle_cpu.py holds to the
    float64 restatement of the blur): the maps are INPUTS of the shade here, whatever made them"""
    m = oracle.shadow_resolve_evsm(depth.astype(np.float32))
    return np.ascontiguousarray(oracle.evsm_blur(m, *radii) if radii else m)


def rgba_of(r: np.ndarray, rng) -> np.ndarray:
    """an RGBA32F map whose red channel is r and whose other channels are other noise: reading .g instead moves every compare"""
    out = noise(rng, r.shape + (4,), -1.0, 2.0)
    out[..., 0] = r
    return np.ascontiguousarray(out)


def light_space(lm, cam_frame, pos):
    """float64: (cascade int[H, W], clip coordinates [H, W, 4] in the pixel's own cascade)"""
    view = np.frombuffer(bytes(cam_frame.view), np.float32).astype(np.float64).reshape(4, 4).T
    p1 = np.concatenate([pos.astype(np.float64), np.ones(pos.shape[:2] + (1,))], -1)
    pv = p1 @ view.T
    depth = np.abs(pv[..., 2] / pv[..., 3])
    c = np.minimum((depth[..., None] >= THRESHOLDS.astype(np.float64)).sum(-1), 3)
    M = lm.astype(np.float64).reshape(4, 4, 4).transpose(0, 2, 1)[c]                     # [H, W, row, column]
    return c, np.einsum("hwrc,hwc->hwr", M, p1)


# ---- the scene family -----------------------------------------------------------------------------------------------------------------------------
def scene(size, matrices="ortho", view="affine", depth="ramp", maps="synth", shadow_type=host.SHADOW_EVSM, map_size=(37, 53), k2_lights=0,
          evsm=("straddle", (2, 5)), penumbra0=False, seed=3, expect=()) -> Case:
    """evsm = (where, blur radii[, below, above]), for maps == "evsm_penumbra" or penumbra0 (beside another map set): cascade 0 from a noise depth image through the EVSM resolve and the blur; `straddle` draws the depths
    from [the fragments' 10 % quantile of light-space depth - below, their 90 % quantile + above], `front` / `behind` wholly beyond / before every
    fragment.  (The (2, 5) case reads a 19 x 13 map over a range that ends at the fragments' 90 % quantile: with 37 x 53 texels and a range of 0.01 either side, the first-order bound of
    oracle_f64.shade left 113 of 6144 pixels out -- nearly shadowed ones, where the factor's relative conditioning is worst -- and the cap is 1 %: the
    case was changed, not the cap.)"""
    W, H = size
    rng = np.random.default_rng(seed)
    cam = synth.make_camera(W, H)
    q = synth.directional_rotation() if matrices != "ortho2" else light_rotation(-35.0, -62.0)
    lm = csm_matrices(cam, q)
    if matrices == "persp":
        lm = projective(lm, (0, 1, 2, 3))
    elif matrices == "persp_one":
        lm = projective(lm, (1,))
    d, sign, boundary = {"ramp": depth_ramp, "checker": depth_checker, "mixed": functools.partial(depth_checker, left_uniform=True),
                         "boundaries": depth_boundaries}[depth](W, H, rng)
    pos = positions_at_depth(cam, d, sign)
    extra = None
    if k2_lights:
        extra = synth.make_lights(cam, d, synth.LightSetConfig(count=k2_lights, spot_fraction=0.3, radius_scale=8.0, d_min=300.0, d_max=9000.0), seed)
        extra["bounds"] = np.float32(4e4)       # every light reaches every pixel well inside its radius window (no 1 - (d / r)^2 cancelling)
    lights = directional_light(synth.directional_forward(q), shadow_type, extra)
    if view == "scaled":
        cam = scaled_view(cam)
    c, clip = light_space(lm, cam.frame, pos)
    assert (clip[..., 3] > 0.25).all(), "w must stay positive"
    if matrices in ("persp", "persp_one"):
        touched = np.isin(c, (0, 1, 2, 3) if matrices == "persp" else (1,))
        assert (clip[..., 3][touched] != 1.0).all() and touched.any()
    lz = clip[..., 2] / clip[..., 3]
    mh, mw = map_size[1], map_size[0]
    ms = synth.make_shadow_set(cam, 64, seed).maps
    out = list(ms)
    centre = [float(np.median(lz[c == k])) if (c == k).any() else 0.5 for k in range(4)]
    if maps in ("pcf_r32f", "pcf_rgba"):
        for k in range(0 if shadow_type != host.SHADOW_EVSM else 1, 4):
            r = noise(rng, (mh, mw), centre[k] - 0.05, centre[k] + 0.05)
            out[k] = r if maps == "pcf_r32f" else rgba_of(r, rng)
    elif maps == "evsm_on_r16f":
        out[0] = noise(rng, (mh, mw), 0.0, 1.0, np.float16)
    if maps == "evsm_penumbra" or penumbra0:
        where, radii = evsm[:2]
        below, above = evsm[2:] if len(evsm) > 2 else (0.01, 0.01)
        z0 = lz[c == 0]
        lo, hi = {"straddle": (np.quantile(z0, 0.1) - below, np.quantile(z0, 0.9) + above), "front": (z0.max() + 0.02, z0.max() + 0.07),
                  "behind": (max(z0.min() - 0.07, 1e-3), z0.min() - 0.02)}[where]
        out[0] = evsm_moments(noise(rng, (mh, mw), lo, hi), radii)
    frame = synth.Frame(f"csm_{depth}", cam, np.ascontiguousarray(d), lights, make_surface(cam, pos, rng, lights),
                        synth.ShadowSet(lights_matrices=np.ascontiguousarray(lm, np.float32), maps=out, size=0))
    return Case(frame, boundary, tuple(expect))


# ---- the direct family ----------------------------------------------------------------------------------------------------------------------------
XY_SHIFT = 8                                  # lp.x = world x * 2^-8, lp.y = world y * 2^-8
Z_BASE = (512.0, 1024.0, 4096.0, 8192.0)      # lp.z = (|world z| - base) * 2^-shift: lp.z = 0 lies strictly inside the cascade's depth range
Z_SHIFT = (9, 9, 11, 13)                      # cascade 0: lp.z in [-1, 0.95); 1: [-0.046, 1.9); 2: [-1.02, 1.25); 3: [-0.18, 1.44)


def direct_matrices() -> np.ndarray:
    lm = np.zeros((4, 4, 4), np.float32)      # [cascade, column, row]
    for c in range(4):
        lm[c, 0, 0] = lm[c, 1, 1] = 2.0 ** -XY_SHIFT
        lm[c, 2, 2] = -(2.0 ** -Z_SHIFT[c])
        lm[c, 3, 2] = -Z_BASE[c] * 2.0 ** -Z_SHIFT[c]
        lm[c, 3, 3] = 1.0
    return lm.reshape(4, 16)


def direct_positions(c, lx, ly, lz) -> np.ndarray:
    """world positions whose clip coordinates in cascade c's direct matrix are (lx, ly, lz, 1); float32, exact where the operands have few bits"""
    base, shift = np.asarray(Z_BASE, np.float32)[c], np.asarray(Z_SHIFT)[c]
    wz = -(base + np.float32(lz) * np.exp2(shift).astype(np.float32))
    return np.stack([np.float32(lx) * np.float32(2.0 ** XY_SHIFT), np.float32(ly) * np.float32(2.0 ** XY_SHIFT), wz], -1).astype(np.float32)


EDGE = np.array([-1 - 2.0 ** -22, -1.0, -1 + 2.0 ** -23, 1 - 2.0 ** -23, 1.0, 1 + 2.0 ** -22], np.float32)
# (px = lp.x / 2 + 1 / 2 and py = 1 - (lp.y / 2 + 1 / 2) of these are floats at every step: -2^-23, 0, 2^-24, 1 - 2^-24, 1, 1 + 2^-23)
Z_EDGE = np.array([-(2.0 ** -23), 0.0, 2.0 ** -22], np.float32)   # pz = lp.z (EVSM) or lp.z / 2 + 1 / 2 (PCF): below, on and above the limit


def direct(size, kind="general", shadow_type=host.SHADOW_EVSM, map_size=(16, 8), missing=(), seed=5, expect=()) -> Case:
    W, H = size
    rng = np.random.default_rng(seed)
    cam = synth.make_camera(W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    q = quadrants(W, H)
    boundary = np.zeros((H, W), bool)
    mw, mh = map_size
    zm = 0.5
    if kind == "reject":
        X = np.concatenate([EDGE, 2.0 * np.array([0.5, 1.0, 3.5, 8.0, 15.5]) / 16.0 - 1.0]).astype(np.float32)   # + texel centres and borders of a 16-wide map
        Y = np.concatenate([EDGE, 2.0 * np.array([0.5, 1.0, 3.5, 4.0, 7.5]) / 8.0 - 1.0]).astype(np.float32)
        Z = np.concatenate([Z_EDGE, np.float32([0.25, 0.625])])
        lx, ly = X[xs % len(X)], Y[ys % len(Y)]
        zi = (xs // len(X) + 4 * (ys // len(Y))) % len(Z)
        lz = Z[zi]
        c = (xs // len(X) + ys // len(Y)) % 4 if shadow_type != host.SHADOW_EVSM else np.where((xs // len(X) + ys // len(Y)) % 2 == 0, 0, 1 + (xs // len(X)) % 3)
        boundary = (xs % len(X) < len(EDGE)) | (ys % len(Y) < len(EDGE)) | (zi < len(Z_EDGE))
    elif kind == "evsm_states":
        # quadrant kinds: 0 every lane far behind the moment (d < 0 on both pairs: the first early return), 1 every lane 0.001 behind (the positive pair's
        # bias 0.003 (1 - ndl) carries a lit pixel past the moment, the negative pair's 0.0001 (1 - ndl) does not: the second early return), 2 every
        # lane in front (neither), 3 the three alternating lane by lane (some)
        k = q % 4
        off = np.array([-0.02, -0.001, 0.02])[np.where(k == 3, (xs + ys) % 3, np.minimum(k, 2))]
        lx, ly = noise(rng, (H, W), -0.9, 0.9), noise(rng, (H, W), -0.9, 0.9)
        lz = (zm + off).astype(np.float32)
        c = np.zeros((H, W), np.int64)
    else:
        lx, ly = noise(rng, (H, W), -1.1, 1.1), noise(rng, (H, W), -1.1, 1.1)
        lz = noise(rng, (H, W), 0.05, 0.9)
        c = np.where(xs < W // 2, q % 4, (q % 3) + ((xs + ys) & 1))                         # `mixed`: both dispatch paths
    pos = direct_positions(c, lx, ly, lz)
    lights = directional_light((0.3, -0.9, 0.2) / np.linalg.norm((0.3, -0.9, 0.2)), shadow_type)
    surface = make_surface(cam, pos, rng, lights)
    if kind == "evsm_states":
        surface[1, ..., :3] = np.float32([0.0, 1.0, 0.0])                                   # ndl about -0.94: lit, 1 - ndl = 1.94 in every lane
        maps0 = evsm_moments(np.full((mh, mw), zm, np.float32))
    else:
        maps0 = evsm_moments(noise(rng, (mh, mw), 0.2, 0.8), (2, 2) if min(mw, mh) > 2 else None)
    if shadow_type != host.SHADOW_EVSM:
        maps0 = rgba_of(noise(rng, (mh, mw), 0.2, 0.8), rng)
    maps = [maps0] + [noise(rng, (mh, mw), 0.2, 0.8, np.float16) for _ in range(3)]
    for k in missing:
        maps[k] = None
    frame = synth.Frame(f"csm_direct_{kind}", cam, np.ascontiguousarray(np.abs(pos[..., 2])), lights, surface,
                        synth.ShadowSet(lights_matrices=direct_matrices(), maps=maps, size=0))
    return Case(frame, boundary, tuple(expect), notes=dict(cascade=c))


def two_level(p: float):
    """The known answer of tests/test_csm_cpu.py: a 4 x 4 cascade-0 map holding the CONSTANT moments of the depth mixture p delta(z1) + (1 - p) delta(z2),
    z1 = 0.3, z2 = 0.5, every pixel of the small frame at light-space depth z2 - 0.0002 under a light that shines straight down on normals that
    point straight up (ndl = -1 exactly, bias = 2).  -> (Case, the same frame's lights / surface for the unshadowed run are the case's own)"""
    W, H = SMALL
    rng = np.random.default_rng(11)
    cam = synth.make_camera(W, H)
    z1, z2 = 0.3, 0.5
    m = np.array([p * np.exp(40 * z1) + (1 - p) * np.exp(40 * z2), p * np.exp(80 * z1) + (1 - p) * np.exp(80 * z2),
                  -(p * np.exp(-40 * z1) + (1 - p) * np.exp(-40 * z2)), p * np.exp(-80 * z1) + (1 - p) * np.exp(-80 * z2)])
    maps = [np.ascontiguousarray(np.broadcast_to(m.astype(np.float32), (4, 4, 4)))] + [np.zeros((4, 4), np.float16) for _ in range(3)]
    lx, ly = noise(rng, (H, W), -0.9, 0.9), noise(rng, (H, W), -0.9, 0.9)
    pos = direct_positions(np.zeros((H, W), np.int64), lx, ly, np.full((H, W), z2 - 0.0002, np.float32))
    lights = directional_light((0.0, -1.0, 0.0), host.SHADOW_EVSM)
    surface = make_surface(cam, pos, rng, lights)
    surface[1, ..., :3] = np.float32([0.0, 1.0, 0.0])
    surface[1, ..., 3] = 1.0
    frame = synth.Frame("csm_two_level", cam, np.ascontiguousarray(np.abs(pos[..., 2])), lights, surface,
                        synth.ShadowSet(lights_matrices=direct_matrices(), maps=maps, size=0))
    return Case(frame, np.zeros((H, W), bool))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
PCF, EVSM = host.SHADOW_PCF, host.SHADOW_EVSM
CASES = {
    # scene family
    "ortho-ramp-synth":            lambda: scene(BIG, expect=("evsm_pos_all", "evsm_neg_some", "pcf_partial", "cascades_all", "mixed_quadrants")),
    "ortho2-ramp-synth-small":     lambda: scene(SMALL, matrices="ortho2", expect=("cascades_all",)),
    "persp-ramp-penumbra_2_5":     lambda: scene(BIG, matrices="persp", maps="evsm_penumbra", map_size=(19, 13), evsm=("straddle", (2, 5), 0.05, 0.0),
                                                 expect=("evsm_pos_some", "evsm_neg_some", "evsm_partial", "cascades_all")),
    "persp-ramp-pcf_r32f-small":   lambda: scene(SMALL, matrices="persp", maps="pcf_r32f", penumbra0=True, map_size=(19, 13), evsm=("straddle", (2, 5), 0.07, 0.0),
                                                 expect=("pcf_partial", "evsm_partial")),
    "persp_one-mixed-penumbra_12": lambda: scene(BIG, matrices="persp_one", depth="mixed", maps="evsm_penumbra", evsm=("straddle", (12, 12), 0.03, 0.01), k2_lights=24,
                                                 expect=("evsm_pos_some", "evsm_neg_some", "evsm_partial", "mixed_quadrants", "uniform_quadrants")),
    "ortho-boundaries-pcf_r32f":   lambda: scene(BIG, depth="boundaries", maps="pcf_r32f", expect=("pcf_partial", "cascades_all")),
    "scaled-checker-pcf_rgba":     lambda: scene(SMALL, view="scaled", depth="checker", maps="pcf_rgba", shadow_type=PCF, expect=("pcf_partial", "mixed_quadrants")),
    "ortho-checker-evsm_on_r16f":  lambda: scene(SMALL, depth="checker", maps="evsm_on_r16f", expect=("mixed_quadrants",)),
    "ortho-ramp-evsm_front":       lambda: scene(BIG, maps="evsm_penumbra", evsm=("front", (2, 5)), expect=("evsm_pos_all", "evsm_neg_all")),
    "ortho-ramp-evsm_behind":      lambda: scene(BIG, maps="evsm_penumbra", evsm=("behind", (2, 5)), expect=("evsm_pos_none", "evsm_neg_none")),
    # direct family
    "reject-evsm":                 lambda: direct(SMALL, "reject", EVSM, expect=("reject_each",)),
    "reject-pcf":                  lambda: direct(SMALL, "reject", PCF, expect=("reject_each",)),
    "evsm_states":                 lambda: direct(SMALL, "evsm_states", EVSM, expect=("evsm_pos_all", "evsm_pos_none", "evsm_pos_some", "evsm_neg_all",
                                                                                         "evsm_neg_none", "evsm_neg_some", "evsm_second_return")),
    "size-16x8":                   lambda: direct(SMALL, expect=("pcf_partial", "mixed_quadrants", "uniform_quadrants")),
    "size-1x1":                    lambda: direct(SMALL, map_size=(1, 1), expect=("mixed_quadrants",)),
    "size-2x2":                    lambda: direct(SMALL, map_size=(2, 2), expect=("pcf_partial",)),
    "size-5x40":                   lambda: direct(SMALL, map_size=(5, 40), expect=("pcf_partial",)),
    "size-64x3":                   lambda: direct(SMALL, map_size=(64, 3), expect=("pcf_partial",)),
    "size-64x3-pcf":               lambda: direct(SMALL, shadow_type=PCF, map_size=(64, 3), expect=("pcf_partial",)),
    "missing-0":                   lambda: direct(SMALL, missing=(0,)),
    "missing-1":                   lambda: direct(SMALL, missing=(1,)),
    "missing-2":                   lambda: direct(SMALL, missing=(2,)),
    "missing-3":                   lambda: direct(SMALL, missing=(3,)),
    "missing-all":                 lambda: direct(SMALL, missing=(0, 1, 2, 3)),
}
MISSING = {"missing-0": (0,), "missing-1": (1,), "missing-2": (2,), "missing-3": (3,), "missing-all": (0, 1, 2, 3)}


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    return CASES[name]()


# ---- references, computed once per case -------------------------------------------------------------------------------------------------------------
def c_oracle(frame, csm=True) -> np.ndarray:
    W, H = frame.cam.width, frame.cam.height
    g, idx, _ = oracle.light_cull(frame.cam.frame, W, H, frame.lights, frame.depth)
    desc = oracle.make_csm(frame.shadows.lights_matrices, frame.shadows.maps) if csm else (None, None)
    return oracle.shade(frame.cam.frame, W, H, frame.surface, frame.lights, g, idx, desc[0])


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(case, float64 radiance, oracle_f64.shade's shadow-margin dict, C oracle radiance)"""
    from oracle import oracle_f64
    case = build(name)
    f = case.frame
    W, H = f.cam.width, f.cam.height
    g, idx, _ = oracle.light_cull(f.cam.frame, W, H, f.lights, f.depth)
    ref, margin = oracle_f64.shade(bytes(f.cam.frame), W, H, f.surface, f.lights, g, idx, (f.shadows.lights_matrices, f.shadows.maps), want_shadow_margin=True)
    return case, ref, margin, c_oracle(f)


def k2_excess(got, ref):
    """err / tol per pixel under the project's K2 bound |got - f64| <= 1e-4 |f64| + 1e-7 max |f64|"""
    err = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
    return (err / (1e-4 * np.abs(ref[..., :3]) + 1e-7 * np.abs(ref[..., :3]).max())).max(-1)


def check_against_float64(got, ref, margin, label=""):
    """the assertions of a fp32 radiance against the float64 reference: the K2 bound on every pixel not left out, the left-out PCF pixels within
    their undecided sixteenths of the unshadowed term, alpha bit for bit -> worst err / tol over the pixels not left out"""
    out = margin["left_out"]
    excess = k2_excess(got, ref)
    assert np.isfinite(got).all(), label
    bad = (excess > 1.0) & ~out
    assert not bad.any(), f"{label}: {bad.sum()} pixels beyond the K2 bound (worst err / tol {excess[~out].max():.2f}), first {np.argwhere(bad)[:5].tolist()}"
    taps = margin["taps_only"]
    err = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
    allow = margin["tap_allowance"] + 1e-4 * np.abs(ref[..., :3]) + 1e-7 * np.abs(ref[..., :3]).max()
    assert (err[taps] <= allow[taps]).all(), f"{label}: a pixel left out for {margin['undecided_taps'][taps].max()} undecided taps is further off than those sixteenths"
    np.testing.assert_array_equal(got[..., 3], ref[..., 3].astype(np.float32))
    return float(excess[~out].max()) if (~out).any() else 0.0


def coverage(case: Case, margin) -> dict:
    """which branches of the shadow term the case reaches, counted on the float64 reference's own decisions of light 0"""
    m = margin["lights"].get(0)
    f = case.frame
    H, W = f.cam.height, f.cam.width
    nq = int(quadrants(W, H).max()) + 1
    if m is None:
        return {}
    by_q = lambda a: a.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(nq, 64)
    casc = by_q(m["cascade"])
    mixed = (casc != casc[:, :1]).any(1)
    cov = {"mixed_quadrants": int(mixed.sum()), "uniform_quadrants": int((~mixed).sum()),
           "cascades_all": int(np.bincount(m["cascade"].ravel(), minlength=4).min()),
           "cascade_pixels": np.bincount(m["cascade"].ravel(), minlength=4).tolist(),
           "reject_pixels": m["rejected"].reshape(-1, 5).sum(0).tolist(),
           "pcf_sixteenths": np.bincount(m["sixteenths"][m["sixteenths"] >= 0].ravel(), minlength=17).tolist()}
    cov["reject_each"] = int(min(cov["reject_pixels"]))
    cov["pcf_partial"] = int(sum(cov["pcf_sixteenths"][1:16]))
    sampled = by_q((m["kind"] == 2) & ~m["rejected"].any(-1))
    whole = sampled.all(1)                                                                # quadrants whose 64 lanes all reach the EVSM look-up
    for i, pair in enumerate(("pos", "neg")):
        dn = by_q(m["d_negative"][..., i])
        cov[f"evsm_{pair}_all"] = int((whole & dn.all(1)).sum())
        cov[f"evsm_{pair}_none"] = int((whole & ~dn.any(1)).sum())
        cov[f"evsm_{pair}_some"] = int((whole & dn.any(1) & ~dn.all(1)).sum())
    cov["evsm_second_return"] = int((whole & ~by_q(m["d_negative"][..., 0]).all(1) & by_q(m["d_negative"][..., 1]).all(1)).sum())
    fac = m["factor"]
    cov["evsm_partial"] = int(((m["kind"] == 2) & (fac > 0.02) & (fac < 0.98)).sum())
    return cov

