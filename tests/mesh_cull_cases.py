"""Placed cases for the instance visibility path (ComputeMeshCulling.shader, ComputeDepthHighZ.shader), shared by tests/test_mesh_cull_cpu.py (the C
oracle against the float64 restatement in oracle/oracle_f64.py) and tests/test_mesh_cull_edges_gpu.py (the kernels against both).

Families (build(name) -> Case, reference(name) -> the float64 dict, coverage(name) -> counts taken from the reference's own decisions):

  exact-*      identity view, models diag(2^k) + integer translations, integer sphere centres: every intermediate of the chain up to the compare is a
               float, so the float64 compare IS the fp32 compare.  The ends of the z range, ProjectSphere's gate and the depth compare, each with the
               tie and the float on either side of it.
  flip-*       one input stepped over adjacent floats across a flip: the four side planes (identity camera and the camera at (0, 150, 0) with a 16:9
               viewport) and m == 2^k.  The level flip is made visible in the flag: the pyramid's odd levels hold 2.0 (in front of every sphere:
               occluded), the even ones 0.0 (never occluded).
  footprint-*  a 16 x 16 x 5 and a 24 x 10 x 5 pyramid under the one-texel probe: the pyramid holds 2.0, above every depthSphere of the case, and one
               texel 0.0; an instance that passes the frustum test and the gate is "not culled" exactly when its footprint holds that texel.
  scene-*      2048-instance clouds under three cameras against pyramids built from synth.make_raw_depth.

Beside them HIZ_SHAPES (pyramid shapes and sources for hiz_build) and the compaction patterns (COMPACT_*), whose keep pattern is made by position:
z = -500 in front of the camera at (0, 150, 0) is kept, z = +5000 behind it is culled -- no flag is written by hand."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle, oracle_f64
from sailor_amd import host, synth

PROBE_FILL, PROBE_HOLE = np.float32(2.0), np.float32(0.0)


@dataclass
class Case:
    frame: object                                 # _lib.UboFrameData
    instances: np.ndarray                         # host.INSTANCE_DTYPE
    hiz: tuple | None                             # (flat float32 pyramid, width, height, levels)
    expect: tuple = ()                            # coverage keys that must be non-zero: what the case exists to reach
    exact: bool = False                           # the float64 reference must be decided on every instance
    probe: bool = False                           # run under the one-texel probe (hiz[0] is the filled pyramid)
    both_outcomes: list = field(default_factory=list)   # slices of instances: the C oracle's flags must hold a 0 and a 1 inside each
    texels: dict = field(default_factory=dict)    # instance index -> number of texels the C oracle's footprint must have (probe cases)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------------------
def identity_frame(width: int = 64, height: int = 64):
    """identity view, fov 90, near 1, far 20000: view-space centre = world centre, cz = -world z; with a square viewport P00 = P11 = 1"""
    world = host.transform_matrix([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0])
    return host.fill_frame_data(world, 90.0, 1.0, 20000.0, width, height)


def records(centres, radii, scale=1.0, translate=(0.0, 0.0, 0.0)) -> np.ndarray:
    """model = translate * diag(scale) (scalars or per instance), sphereBounds = (centre, radius); materialInstance = the index"""
    centres = np.asarray(centres, np.float32).reshape(-1, 3)
    n = len(centres)
    inst = np.zeros(n, host.INSTANCE_DTYPE)
    model = np.zeros((n, 16), np.float32)
    sc = np.broadcast_to(np.asarray(scale, np.float32), (n,))
    model[:, 0] = sc; model[:, 5] = sc; model[:, 10] = sc; model[:, 15] = 1.0
    model[:, 12:15] = np.broadcast_to(np.asarray(translate, np.float32), (n, 3))
    inst["model"] = model
    inst["sphereBounds"][:, :3] = centres
    inst["sphereBounds"][:, 3] = np.broadcast_to(np.asarray(radii, np.float32), (n,))
    inst["materialInstance"] = np.arange(n, dtype=np.uint32)
    inst["isCulled"] = 7
    return inst


def concat(*parts) -> np.ndarray:
    out = np.concatenate([p.view(np.uint8).reshape(-1, 96) for p in parts]).reshape(-1).view(host.INSTANCE_DTYPE)
    out["materialInstance"] = np.arange(len(out), dtype=np.uint32)
    return out


def step_floats(x, steps) -> np.ndarray:
    """the floats `steps` (ints) places away from float32 x, in the order of the reals"""
    bits = np.float32(x).view(np.int32).astype(np.int64)
    key = np.where(bits < 0, -(bits & 0x7FFFFFFF), bits) + np.asarray(steps, np.int64)     # a monotone integer key of the floats
    back = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return back.view(np.float32)


def constant_pyramid(width, height, levels, value) -> tuple:
    return np.full(oracle.hiz_level_offsets(width, height, levels)[1], value, np.float32), width, height, levels


def parity_pyramid(width, height, levels) -> tuple:
    """odd levels 2.0 (occludes every sphere with depthSphere < 2), even levels 0.0 (occludes none): the flag shows the level's parity"""
    offs, total = oracle.hiz_level_offsets(width, height, levels)
    p = np.zeros(total, np.float32)
    for l in range(1, levels, 2):
        p[offs[l]:(offs[l + 1] if l + 1 < levels else total)] = 2.0
    return p, width, height, levels


# ---- exact-* -----------------------------------------------------------------------------------------------------------------------------------
def _exact_z():
    # far end: cz - r > 20000 culls.  cz = 20003 (+- one float = 2^-9), r = 3: the difference is a float, 20000 is the tie (kept)
    far = step_floats(20003.0, [-1, 0, 1])
    a = records(np.stack([np.zeros(3), np.zeros(3), -far], 1), 3.0)
    # the same through diag(2) and a translation: centre z = 2 * -10000 - 3 (+ the stepped part in the translation)
    b = records([[0, 0, -10000.0]] * 3, 1.5, scale=2.0, translate=np.stack([np.zeros(3), np.zeros(3), -(far - np.float32(20000.0))], 1))
    # near end: cz + r < 1 culls.  cz = -2 (behind the eye), r = 3: the sum is 1 (kept); the floats beside -2, and cz = -2.5 (0.5: culled)
    near = step_floats(-2.0, [-1, 0, 1])
    c = records(np.stack([np.zeros(3), np.zeros(3), -near], 1), 3.0)
    d = records([[0, 0, 2.5], [0, 0, -20004.0]], 3.0)                       # cz + r = 0.5 and cz - r = 20001: culled
    e = records([[0, 0, 4.0]] * 3, 6.0, scale=0.5, translate=np.stack([np.zeros(3), np.zeros(3), -(near + np.float32(2.0)) ], 1))
    # the pyramid holds 0.0: nothing is occluded, the flag is the frustum test's alone
    return Case(identity_frame(), concat(a, b, c, d, e), constant_pyramid(16, 16, 5, 0.0), exact=True,
                expect=("z_far_true", "z_far_false", "z_near_true", "z_near_false", "tie_z_far", "tie_z_near", "gate_false"))


def _exact_gate():
    # C.z < r + znear: (0, 0, -4), r = 3 is the tie (the gate passes, depthSphere = 1 < 2.0: occluded); the float below 4 fails the gate (kept)
    z = step_floats(4.0, [-1, 0, 1])
    a = records(np.stack([np.zeros(3), np.zeros(3), -z], 1), 3.0)
    b = records([[0, 0, -1.0]] * 3, 1.5, scale=2.0, translate=np.stack([np.zeros(3), np.zeros(3), -(z - np.float32(2.0))], 1))
    return Case(identity_frame(), concat(a, b), constant_pyramid(16, 16, 5, 2.0), exact=True, both_outcomes=[slice(0, 3), slice(3, 6)],
                expect=("gate_true", "gate_false", "tie_gate", "depth_true"))


def _exact_depth(which):
    # depthSphere = 1 / (7 - 3) = 0.25 against a pyramid of 0.25 (tie: not occluded), the float above it (occluded) and the float below (not)
    value = step_floats(0.25, [{"below": -1, "tie": 0, "above": 1}[which]])[0]
    a = records([[0, 0, -7.0], [0, 0, -9.0], [0, 0, -5.0]], [3.0, 5.0, 1.0])
    b = records([[0, 0, -3.5]], 1.5, scale=2.0)
    c = records([[0, 0, -6.0]], 3.0, translate=(0.0, 0.0, -1.0))
    return Case(identity_frame(), concat(a, b, c), constant_pyramid(16, 16, 5, value), exact=True,
                expect=(("depth_true",) if which == "above" else ("depth_false",)) + (("tie_depth",) if which == "tie" else ()))


# ---- flip-* ------------------------------------------------------------------------------------------------------------------------------------
PLANE_STEPS = np.concatenate([[-65536, -4096, -256], np.arange(-24, 25), [256, 4096, 65536]])   # adjacent floats across the flip, and a few the bound decides


def _flip_planes(frame, cam_y):
    """per side plane a sphere whose centre sits where dot(n, c) == -r, one world coordinate stepped over 49 adjacent floats (and six farther ones)"""
    fr = oracle_f64.frame_fields(bytes(frame))
    normals, _ = oracle_f64.view_frustum_margin(fr)
    parts, groups, at = [], [], 0
    for p in range(4):
        for depth, r in ((100.0, 10.0), (3000.0, 61.0)):
            base = np.array([0.0, 0.0, depth])
            c = base - (normals[p] @ base + r) * normals[p]                  # view space, z forward: dot(n, c) = -r
            world = np.array([c[0], c[1] + cam_y, -c[2]])
            axis = int(np.argmax(np.abs(normals[p][:2])))                    # x for left / right, y for top / bottom
            w = np.repeat(world.astype(np.float32)[None], len(PLANE_STEPS), 0)
            w[:, axis] = step_floats(np.float32(world[axis]), PLANE_STEPS)
            parts.append(records(np.zeros((len(w), 3)), r, translate=w))
            groups.append(slice(at, at + len(w))); at += len(w)
    return Case(frame, concat(*parts), None, both_outcomes=groups, expect=tuple(f"plane{p}_{o}" for p in range(4) for o in ("true", "false")))


def _plane_tie():
    """dot(n, c) - w < -r at an exact tie: with the identity camera and a square viewport the side normals are (+-a, 0, a) and (0, +-a, a) with ONE
    float a, so a centre (-+d, 0, d) or (0, -+d, d) has n.x c.x + n.z c.z == 0 exactly in any evaluation, and a sphere of radius 0 makes the compare
    0 < -0: false, kept.  One float farther out the dot product is negative: culled.  (The float64 bound cannot know that the two products cancel, so
    these instances are left undecided there; the tie is asserted on the flags themselves.)"""
    parts, groups, at = [], [], 0
    for axis, sign in ((0, -1.0), (0, 1.0), (1, -1.0), (1, 1.0)):
        for d in (50.0, 3.0):
            c = np.zeros((3, 3), np.float32)
            c[:, 2] = -d
            c[:, axis] = step_floats(sign * d, [-1, 0, 1])
            parts.append(records(c, 0.0))
            groups.append(slice(at, at + 3)); at += 3
    return Case(identity_frame(), concat(*parts), None, both_outcomes=groups, expect=("plane0_true", "plane1_true", "plane2_true", "plane3_true"))


LEVEL_STEPS = np.arange(-64, 65)


def _flip_level(frame, W, H, levels, cam_y, centre):
    """for every k a radius at which max(width, height) == 2^k (bisected on the float64 reference), stepped over 129 adjacent floats"""
    hiz = parity_pyramid(W, H, levels)
    c = np.float32([centre[0], centre[1] + cam_y, centre[2]])

    def m_of(r):
        return oracle_f64.mesh_cull_flags(bytes(frame), records([[0, 0, 0]], r, translate=c), hiz)["m"][0]

    parts, groups, at = [], [], 0
    for k in range(1, levels):
        lo, hi = 1e-3, float(-centre[2]) - 1.5
        assert m_of(lo) < 2.0 ** k < m_of(hi), (k, m_of(lo), m_of(hi))
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if m_of(np.float32(mid)) < 2.0 ** k else (lo, mid)
        parts.append(records(np.zeros((len(LEVEL_STEPS), 3)), step_floats(np.float32(hi), LEVEL_STEPS), translate=c))
        groups.append(slice(at, at + len(LEVEL_STEPS))); at += len(LEVEL_STEPS)
    return Case(frame, concat(*parts), hiz, both_outcomes=groups, expect=tuple(f"level{l}" for l in range(levels)) + ("pow2_near",))


# ---- footprint-* -------------------------------------------------------------------------------------------------------------------------------
def _special_models() -> np.ndarray:
    """a negative radius, a zero-scale model, w == 0 in the model (Inf and NaN centres), m[15] = 2"""
    a = records([[0, 0, -5.0], [0, 0, -5.0], [1.0, 2.0, 0.0], [0, 0, 0], [0, 0, -10.0]], [-3.0, 3.0, 3.0, 3.0, 3.0])
    a["model"][1, [0, 5, 10]] = 0.0; a["model"][1, 12:15] = [0.0, 0.0, -5.0]        # zero scale: radius 0, the centre is the translation
    a["model"][2, 15] = 0.0                                                          # w == 0: the centre is (Inf, Inf, NaN)
    a["model"][3, 15] = 0.0                                                          # 0 / 0: the centre is NaN
    a["model"][4, 15] = 2.0                                                          # w == 2: the centre is halved, (0, 0, -5), the radius is not
    return a


def _footprint(W, H, levels):
    edges = [(sx * 34.0, sy * 34.0, -31.0) for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1))]
    parts = [
        records([[0, 0, -5.0], [30, 0, -31.0]], [3.0, 2.0]),                         # on the axis (3-4-5: exact), the right edge
        records([[0, 0, -50.0]] * 7, [0.01, 3.0, 4.5, 9.0, 15.0, 25.0, 40.0]),       # on the axis, every level: texel-centre hits where a level's size is odd
        records([[0, 0.7, -50.0]] * 3 + [[0.7, 0, -50.0]] * 3, [4.5, 25.0, 40.0] * 2),  # off the axis in y only / in x only: a centre hit on one axis
        records(edges, 3.0),                                                         # uv beyond each edge and each corner
        records([[0, 0, -21.0], [0, 0, -60.0]], [20.0, 58.9]),                       # m >= 2^levels: the top level by clamp
        records([[7.0, -3.0, -90.0], [-11.0, 5.0, -40.0], [2.5, 2.5, -12.0]], [0.02, 6.0, 4.0]),
        _special_models(),
    ]
    inst = concat(*parts)
    expect = ("level0_clamp", "top_clamp", "m_below_1", "m_nonpositive", "texels_1", "texels_2", "texels_4", "frac0_both",
              "edge_left", "edge_right", "edge_top", "edge_bottom", "corner", "centre_inf", "centre_nan", "uv_outside")
    if W == 16:   # every level of 16 x 16 but the last is even-sized: a centre hit (u = 0.5) needs the 1 x 1 level, where it is a hit on both axes
        texels = {0: 4, 1: 2}                                                        # level 3 whole; two level-0 texels at the right edge
    else:         # 24 x 10: level 1 is 12 x 5 (y hits a centre on the axis), level 3 is 3 x 1 (x does)
        expect += ("frac0_x_only", "frac0_y_only")
        texels = {4: 2, 7: 1}                                                        # on the axis at level 1: two columns, one row; at level 3: one texel
    return Case(identity_frame(), inst, constant_pyramid(W, H, levels, PROBE_FILL), probe=True, expect=expect, texels=texels)


# ---- scene-* -----------------------------------------------------------------------------------------------------------------------------------
def _scene(width, height, fov, levels, seed):
    cam = synth.make_camera(width, height, fov=fov)
    raw = synth.make_raw_depth(synth.make_linear_depth(width // 2, height // 2, seed, d_min=200.0, d_max=2500.0), cam.frame.cameraZNearZFar[0])
    side = width // 2
    pyr = oracle.hiz_build(raw, side, side, levels)          # DefaultRenderer.renderer: DepthHighZ is ViewportWidth / 2 squared
    s = synth.make_instance_set(2048, 1, seed=synth.SEED + seed)
    return Case(cam.frame, s.instances, (pyr, side, side, levels), expect=("frustum_true", "frustum_false", "gate_true", "depth_true", "depth_false"))


_BUILDERS = {
    "exact-zrange": _exact_z,
    "exact-gate": _exact_gate,
    "exact-depth-below": lambda: _exact_depth("below"),
    "exact-depth-tie": lambda: _exact_depth("tie"),
    "exact-depth-above": lambda: _exact_depth("above"),
    "flip-plane-tie-zero-radius": _plane_tie,
    "flip-planes-identity": lambda: _flip_planes(identity_frame(), 0.0),
    "flip-planes-camera": lambda: _flip_planes(synth.make_camera(1920, 1080).frame, 150.0),
    "flip-level-16x16": lambda: _flip_level(identity_frame(), 16, 16, 5, 0.0, (0.0, 0.0, -50.0)),
    "flip-level-camera-24x10": lambda: _flip_level(synth.make_camera(1920, 1080).frame, 24, 10, 5, 150.0, (3.0, -2.0, -80.0)),
    "footprint-16x16": lambda: _footprint(16, 16, 5),
    "footprint-24x10": lambda: _footprint(24, 10, 5),
    "scene-1080p": lambda: _scene(1920, 1080, 90.0, 10, 5),
    "scene-720p-fov50": lambda: _scene(1280, 720, 50.0, 9, 6),
    "scene-360p": lambda: _scene(640, 360, 70.0, 7, 7),
}
NAMES = tuple(_BUILDERS)
PROBE_NAMES = tuple(n for n in NAMES if n.startswith("footprint-"))


@functools.lru_cache(maxsize=None)
def build(name: str) -> Case:
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    case = build(name)
    return oracle_f64.mesh_cull_flags(bytes(case.frame), case.instances, case.hiz)


@functools.lru_cache(maxsize=None)
def oracle_flags(name: str) -> np.ndarray:
    """the C oracle's isCulled per instance (computed once, shared by the CPU and the GPU tests)"""
    case = build(name)
    if case.hiz is None:
        return oracle.mesh_frustum_cull(case.frame, case.instances)["isCulled"].copy()
    return oracle.mesh_cull_occlusion(case.frame, case.instances, *case.hiz)["isCulled"].copy()


def probe_pyramid(case: Case, texel: int) -> np.ndarray:
    p = case.hiz[0].copy()
    p[texel] = PROBE_HOLE
    return p


@functools.lru_cache(maxsize=None)
def oracle_probe_survivors(name: str) -> np.ndarray:
    """bool[texels, instances]: the C oracle leaves the instance unculled under the probe of that texel"""
    case = build(name)
    _, W, H, levels = case.hiz
    return np.stack([oracle.mesh_cull_occlusion(case.frame, case.instances, probe_pyramid(case, t), W, H, levels)["isCulled"] == 0
                     for t in range(len(case.hiz[0]))])


def reference_probe_survivors(name: str) -> np.ndarray:
    """the same from the float64 reference's footprints: unculled = passes the frustum test and (fails the gate, or the hole is in the footprint, or
    depthSphere is not below the fill value)"""
    case, ref = build(name), reference(name)
    t = np.arange(len(case.hiz[0]))
    hit = (ref["footprint"][None, :, :] == t[:, None, None]).any(-1)
    with np.errstate(invalid="ignore"):
        behind_fill = ref["depth_sphere"] < float(PROBE_FILL)
        behind_hole = ref["depth_sphere"] < float(PROBE_HOLE)
    occluded = ref["gate"][None, :] & np.where(hit, behind_hole[None, :], behind_fill[None, :])
    return ~(ref["frustum"][None, :] | occluded)


COVERAGE_KEYS = (("frustum_true", "frustum_false", "z_far_true", "z_far_false", "z_near_true", "z_near_false", "tie_z_far", "tie_z_near")
                 + tuple(f"plane{p}_{o}" for p in range(4) for o in ("true", "false"))
                 + ("gate_true", "gate_false", "tie_gate", "depth_true", "depth_false", "tie_depth", "pow2_near")
                 + tuple(f"level{l}" for l in range(5))
                 + ("level0_clamp", "top_clamp", "m_below_1", "m_nonpositive", "texels_1", "texels_2", "texels_4", "frac0_x_only", "frac0_y_only", "frac0_both",
                    "edge_left", "edge_right", "edge_top", "edge_bottom", "corner", "uv_outside", "centre_inf", "centre_nan"))


def coverage(name: str) -> dict:
    """what the case reaches, counted on the float64 reference's own decisions"""
    case, ref = build(name), reference(name)
    cov = {k: 0 for k in COVERAGE_KEYS}
    cnt = lambda m: int(np.count_nonzero(m))
    cov["frustum_true"], cov["frustum_false"] = cnt(ref["frustum"]), cnt(~ref["frustum"])
    cov["z_far_true"], cov["z_far_false"] = cnt(ref["z_out"][:, 0]), cnt(~ref["z_out"][:, 0])
    cov["z_near_true"], cov["z_near_false"] = cnt(ref["z_out"][:, 1]), cnt(~ref["z_out"][:, 1])
    cov["tie_z_far"], cov["tie_z_near"] = cnt(ref["q_z"][:, 0] == 0), cnt(ref["q_z"][:, 1] == 0)
    in_z = ~ref["z_out"].any(-1)
    for p in range(4):
        cov[f"plane{p}_true"], cov[f"plane{p}_false"] = cnt(ref["plane_out"][:, p] & in_z), cnt(~ref["plane_out"][:, p] & in_z)
    if case.hiz is None:
        return cov
    levels = case.hiz[3]
    live = ~ref["frustum"]
    gate = live & ref["gate"]
    cov["gate_true"], cov["gate_false"], cov["tie_gate"] = cnt(gate), cnt(live & ~ref["gate"]), cnt(live & (ref["q_gate"] == 0))
    cov["depth_true"], cov["depth_false"] = cnt(gate & ref["occluded"]), cnt(gate & ~ref["occluded"])
    cov["tie_depth"] = cnt(gate & (ref["q_depth"] == 0))
    with np.errstate(invalid="ignore"):
        m = ref["m"]
        cov["pow2_near"] = cnt(gate & (ref["d_pow2"] < 1e-5 * np.abs(m)))
        for l in range(min(levels, 5)):
            cov[f"level{l}"] = cnt(gate & (ref["level"] == l))
        cov["level0_clamp"] = cnt(gate & ~(ref["level_raw"] >= 0))
        cov["top_clamp"] = cnt(gate & (ref["level_raw"] > levels - 1))
        cov["m_below_1"] = cnt(gate & (m > 0) & (m < 1))
        cov["m_nonpositive"] = cnt(gate & (m <= 0))
        sizes = np.array([len(s) for s in oracle_f64.footprint_sets(ref["footprint"])])
        for k in (1, 2, 4):
            cov[f"texels_{k}"] = cnt(gate & (sizes == k))
        fx0, fy0 = ref["fx"]["frac"] == 0, ref["fy"]["frac"] == 0
        cov["frac0_x_only"], cov["frac0_y_only"], cov["frac0_both"] = cnt(gate & fx0 & ~fy0), cnt(gate & ~fx0 & fy0), cnt(gate & fx0 & fy0)
        wl, hl = ref["level_size"][:, 0], ref["level_size"][:, 1]
        x, y = ref["fx"]["x"], ref["fy"]["x"]
        left, right, top, bottom = x < 0, x > wl - 1, y < 0, y > hl - 1
        multi = (wl > 1) & (hl > 1)
        cov["edge_left"], cov["edge_right"] = cnt(gate & left & multi), cnt(gate & right & multi)
        cov["edge_top"], cov["edge_bottom"] = cnt(gate & top & multi), cnt(gate & bottom & multi)
        cov["corner"] = cnt(gate & (left | right) & (top | bottom) & multi)
        uv = ref["uv"]
        cov["uv_outside"] = cnt(gate & ((uv < 0) | (uv > 1)).any(-1))
        cov["centre_inf"] = cnt(np.isinf(ref["center"]).any(-1))
        cov["centre_nan"] = cnt(np.isnan(ref["center"]).any(-1))
    return cov


# ---- Hi-Z shapes -------------------------------------------------------------------------------------------------------------------------------
# (name, source (rows, columns), pyramid width, height, levels, source kind, per level (columns, rows) whose fp32 sample position takes another
# footprint than the exact one -- a fact of the fp32 evaluation of (i + 0.5) / dst * src - 0.5, None = not pinned)
HIZ_SHAPES = (
    ("shipped-960", (540, 960), 960, 960, 10, "depth", [(25, 0)] + [(0, 0)] * 9),
    ("same-131", (67, 131), 131, 131, 8, "depth", [(2, 0)] + [(0, 0)] * 7),
    ("same-96", (54, 96), 96, 96, 7, "depth", [(0, 0)] * 7),
    ("pow2-64", (64, 64), 64, 64, 7, "depth", [(0, 0)] * 7),
    ("three-to-one-48", (48, 48), 16, 16, 5, "depth", [(0, 0)] * 5),
    ("three-to-one-36", (36, 36), 12, 12, 4, "depth", [(0, 0)] * 4),
    ("non-integer-ratio", (67, 131), 50, 30, 6, "depth", None),
    ("one-row", (1, 37), 37, 1, 7, "depth", None),
    ("one-column", (41, 1), 1, 41, 7, "depth", None),
    ("one-texel-source", (1, 1), 4, 4, 3, "depth", None),
    ("x-reaches-one-first", (64, 4), 4, 64, 8, "depth", None),           # levels past 1 x 1
    ("y-reaches-one-first", (4, 64), 64, 4, 8, "depth", None),
    ("one-level", (30, 50), 25, 15, 1, "depth", None),
    ("sixteen-levels", (8, 8), 8, 8, 16, "depth", None),
    ("tail-at-64x64", (256, 256), 128, 128, 8, "depth", [(0, 0)] * 8),   # the level built from 64 x 64 starts the one-launch tail
    ("tail-after-65x10", (40, 260), 130, 20, 8, "depth", None),          # 65 x 10 is not taken by the tail, 32 x 5 is
    ("tail-after-20x200", (400, 40), 20, 200, 9, "depth", None),         # only one side <= 64 until 5 x 50
    ("source-inf", (24, 40), 20, 12, 5, "inf", None),
    ("source-zeros", (24, 40), 20, 12, 5, "zeros", None),
    ("source-nan", (24, 40), 20, 12, 5, "nan", None),
)
HIZ_NAMES = tuple(s[0] for s in HIZ_SHAPES)


@functools.lru_cache(maxsize=None)
def hiz_source(name: str):
    """-> (raw depth float32[rows, columns], width, height, levels, pinned convention counts or None)"""
    _, (rows, cols), W, H, levels, kind, counts = HIZ_SHAPES[HIZ_NAMES.index(name)]
    raw = synth.make_raw_depth(synth.make_linear_depth(cols, rows, 5, d_min=200.0, d_max=2500.0), 1.0).copy()
    u = synth.uniforms(synth.STREAM_DEPTH, rows * cols, 1 << 23).reshape(rows, cols)
    if kind == "inf":
        raw[u < 0.2] = np.inf
    elif kind == "zeros":                                                  # 0.0 = nothing drawn; -0.0 compares equal to it
        raw[u < 0.3] = 0.0
        raw[u < 0.15] = -0.0
    elif kind == "nan":
        raw[u < 0.1] = np.nan
    return raw, W, H, levels, counts


@functools.lru_cache(maxsize=None)
def hiz_oracle(name: str) -> np.ndarray:
    raw, W, H, levels, _ = hiz_source(name)
    return oracle.hiz_build(raw, W, H, levels)


# ---- compaction patterns -----------------------------------------------------------------------------------------------------------------------
COMPACT_COUNTS = (0, 1, 255, 256, 257, 511, 512, 513, 64 * 256, 64 * 256 + 1, 65 * 256 + 1)
COMPACT_PATTERNS = ("all", "none", "alternating", "only-first", "only-last", "last-of-first-chunk", "one-chunk", "prefix")
COMPACT_BATCH_NUMBERS = (1, 1023, 1024, 1025, 2049)


def keep_pattern(pattern: str, count: int) -> np.ndarray:
    """bool[count].  only-last is also "only the last record of the last chunk"; one-chunk keeps everything in the middle 256-record chunk only"""
    i = np.arange(count)
    if pattern == "all":
        return np.ones(count, bool)
    if pattern == "none":
        return np.zeros(count, bool)
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "only-first":
        return i == 0
    if pattern == "only-last":
        return i == count - 1
    if pattern == "last-of-first-chunk":
        return i == min(255, count - 1)
    if pattern == "one-chunk":
        return i // 256 == ((count - 1) // 256) // 2
    if pattern == "prefix":
        return i < (count + 2) // 3
    raise KeyError(pattern)


def compact_camera():
    return synth.make_camera(1920, 1080)


def compact_records(keep: np.ndarray) -> np.ndarray:
    """kept records stand at (0, 150, -500) in front of the camera, culled ones at (0, 150, 5000) behind it"""
    z = np.where(keep, np.float32(-500.0), np.float32(5000.0)).astype(np.float32)
    w = np.stack([np.zeros(len(keep), np.float32), np.full(len(keep), 150.0, np.float32), z], 1)
    return records(np.zeros((len(keep), 3)), 10.0, translate=w)


def batches_of(firsts, counts) -> np.ndarray:
    b = np.zeros((len(firsts), 5), np.uint32)
    b[:, 0] = 36 + 3 * (np.arange(len(firsts)) % 100); b[:, 1] = counts; b[:, 2] = 1000 * np.arange(len(firsts)); b[:, 3] = np.arange(len(firsts)); b[:, 4] = firsts
    return b


def compact_single(count: int, pattern: str):
    """one batch over `count` records -> (instances, batches); the empty draw owns none of a one-record buffer (an instance buffer is never empty)"""
    if count == 0:
        return compact_records(np.ones(1, bool)), batches_of([0], [0])
    return compact_records(keep_pattern(pattern, count)), batches_of([0], [count])


def compact_many(num_batches: int):
    """ragged contiguous batches (sizes 0..40 in a fixed cycle, a 700-record one in the middle), the alternating-by-three keep pattern"""
    sizes = (np.arange(num_batches) * 7) % 41
    sizes[num_batches // 2] = 700
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    total = int(sizes.sum())
    return compact_records(np.arange(total) % 3 != 1), batches_of(firsts, sizes)


def compact_gaps():
    """batches with gaps between them, in non-ascending firstInstance order; the window is the whole buffer, so gap records get their flag and
    nothing else"""
    total = 6000
    keep = (np.arange(total) * 5) % 7 < 3
    return compact_records(keep), batches_of([5000, 100, 3000, 10, 900], [700, 300, 513, 50, 0])


def compact_expected(frame, inst: np.ndarray, batches: np.ndarray):
    """step 2 by the C oracle's flags, step 3 by the NumPy partition -> (words uint32[n, 24], batches)"""
    words = inst.view(np.uint32).reshape(-1, 24).copy()
    words[:, 21] = oracle.mesh_frustum_cull(frame, inst)["isCulled"]
    return oracle_f64.compact_partition(words, batches)
