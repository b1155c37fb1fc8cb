"""The scenes of the Transparent-queue tests (tests/test_transparent_cpu.py, tests/test_transparent_gpu.py): frames of 48 x 32 and 50 x 35 (a ragged tile column and
row) under the synthetic camera, at most 16 triangles a scene, six point lights.  A scene is tests/transparent_ref.py's dict -- a draw carries `blend` -- plus
`opaque` (the draws of the prepass that left the depth attachment), `cam` and `lights`.  CASES maps a name to (builder, predicate(layers, stats, scene)): the
predicate states what the case was built to reach, so that it cannot silently stop reaching it."""
import numpy as np

import surface_cases as sc
from gltf_cases import gltf, gltf_material
from masked_cases import checker, cutout
from sailor_amd import host, synth
from surface_cases import FLAT_NORMAL, IDENTITY, WHITE, draw, material, vertex

f32 = np.float32
EYE = np.array([0.0, 150.0, 0.0])   # synth.make_camera's position; it looks down -z, fov 90 degrees, near plane 1


def blended(d, mode):
    d = dict(d)
    d["blend"] = mode
    return d


def wall(W, H, d, x0=-1.3, y0=-1.3, x1=1.3, y1=1.3, d1=None, color=(1, 1, 1, 1), colors=None, uv=((0, 0), (1, 0), (1, 1), (0, 1))):
    """a rectangle facing the camera: its corners at the normalised device coordinates (x0, y0) .. (x1, y1), at distance d (d1: the distance of its right
    edge, for a slanted one) -> (vertices, the two triangles)"""
    d1 = d if d1 is None else d1
    corners = [(x0, y0, d), (x1, y0, d1), (x1, y1, d1), (x0, y1, d)]
    colors = [color] * 4 if colors is None else colors
    return [vertex((EYE[0] + x * q * W / H, EYE[1] + y * q, EYE[2] - q), uv[k], colors[k]) for k, (x, y, q) in enumerate(corners)], [(0, 1, 2), (0, 2, 3)]


def along_the_ray(vertices, factor):
    """every vertex moved along its ray from the eye: the same pixels, another depth"""
    out = np.array(vertices, f32).reshape(-1, 18).copy()
    out[:, 2:5] = (EYE + (out[:, 2:5].astype(np.float64) - EYE) * factor).astype(f32)
    return out


def lights():
    rng = np.random.default_rng(23)
    l = np.zeros(6, host.LIGHT_DTYPE)
    l["worldPosition"] = np.stack([rng.uniform(-50, 50, 6), rng.uniform(135, 160, 6), rng.uniform(-60, -5, 6)], 1).astype(f32)
    l["bounds"] = np.repeat(rng.uniform(80, 140, 6).astype(f32)[:, None], 3, axis=1)
    l["intensity"] = rng.uniform(40, 250, (6, 3)).astype(f32)
    l["attenuation"] = np.array([1.0, 0.022, 0.0019], f32)
    l["cutOff"] = np.array(host.cutoff_cosines(30.0, 45.0), f32)
    l["direction"] = np.array([0, -1, 0], f32)
    l["type"], l["shadowType"] = host.LIGHT_POINT, host.SHADOW_PCF
    return l


def cam_scene(W, H, draws, opaque=None, models=(IDENTITY,), **kw):
    cam = synth.make_camera(W, H)
    fb = np.frombuffer(bytes(cam.frame), f32)
    s = sc.scene(W, H, fb[16:32].copy(), draws, models=models, view=fb[0:16].copy(), **kw)
    back = wall(W, H, 100.0, x0=-0.4)   # the opaque pass left a wall behind the right two thirds of the frame; the rest is the far plane (depth 0)
    s["opaque"] = [draw(back[0], back[1], ids=[0])] if opaque is None else opaque
    s["cam"], s["lights"] = cam, lights()
    return s


def depth_attachment(s):
    """what the prepass and the opaque passes left: the project's oracle over the opaque draws"""
    return sc.prepass_depth(dict(s, draws=s["opaque"]))


MATS = [material(albedo=(0.9, 0.3, 0.2, 0.5), metallic=0.3, roughness=0.7), material(albedo=(0.2, 0.8, 0.3, 0.25), metallic=0.1, roughness=0.5),
        material(albedo=(0.2, 0.3, 0.9, 0.75), metallic=0.6, roughness=0.9)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def order_abc(W=48, H=32):
    """three overlapping quads drawn A, B, C under AlphaBlending at distances 60, 50, 70: the depth order (C behind A behind B) is not the draw order"""
    a, b, c = wall(W, H, 60.0, -0.8, -0.7, 0.4, 0.5), wall(W, H, 50.0, -0.3, -0.4, 0.9, 0.8), wall(W, H, 70.0, -0.6, -0.2, 0.6, 0.9)
    return cam_scene(W, H, [blended(draw(q[0], q[1], ids=[k]), "alpha") for k, q in enumerate((a, b, c))], models=[IDENTITY] * 3, mats=MATS, inst_materials=[0, 1, 2])


def depth_edge(W=50, H=35):
    """the very triangle of the prepass (equal bits pass), one a hair behind it (fails everywhere), one in front (passes)"""
    q = wall(W, H, 70.0, -0.7, -0.8, 0.8, 0.6, d1=55.0)
    tri = np.array(q[0][:3], f32)
    same = draw(tri, [(0, 1, 2)], ids=[0])
    return cam_scene(W, H, [blended(same, "alpha"), blended(draw(along_the_ray(tri, 1.0001), [(0, 1, 2)], ids=[1]), "additive"),
                            blended(draw(along_the_ray(tri, 0.999), [(0, 1, 2)], ids=[2]), "alpha")],
                     opaque=[same], models=[IDENTITY] * 3, mats=MATS, inst_materials=[0, 1, 2])


def self_overlap(W=48, H=32):
    """a closed cube without culling (front and back faces in ONE draw) and two instances of one quad exactly over each other"""
    v, t = synth.face_cube_mesh()
    cube = host.transform_matrix([-12.0, 152.0, -45.0, 1.0], (lambda q: q / np.linalg.norm(q))(np.array([0.2, 0.4, 0.1, 0.9])), [9.0, 8.0, 7.0, 1.0])
    q = wall(W, H, 40.0, -0.3, -0.6, 0.9, 0.7)
    return cam_scene(W, H, [blended(draw(v, t, ids=[0]), "alpha"), blended(draw(q[0], q[1], ids=[1, 2]), "additive")], models=[cube, IDENTITY, IDENTITY],
                     mats=MATS, inst_materials=[0, 1, 2])


def near_cut(W=50, H=35):
    """a triangle with one vertex beyond the near plane (the cut leaves a quad: two parts) over a quad"""
    col = [(1, 0.5, 0.5, 0.5), (0.5, 1, 0.5, 0.75), (0.5, 0.5, 1, 1)]
    tri = [vertex((-1.5 + 0.8, 150.0 - 0.5, -3.0), (0, 0), col[0]), vertex((-0.2 + 0.8, 150.0 - 0.7, -0.4), (1, 0), col[1]), vertex((-0.9 + 0.8, 150.0 + 0.8, -2.5), (0, 1), col[2])]
    q = wall(W, H, 30.0, -0.9, -0.9, 0.9, 0.9)
    return cam_scene(W, H, [blended(draw(q[0], q[1], ids=[0]), "alpha"), blended(draw(tri, [(0, 2, 1)], ids=[1]), "alpha")], models=[IDENTITY] * 2,
                     mats=[material(albedo=(0.9, 0.3, 0.2, 0.5), metallic=0.3, roughness=0.7), material(albedo=(1, 1, 1, 1), metallic=0.2, roughness=0.8)],
                     inst_materials=[0, 1])


def mixed_modes(W=48, H=32):
    """Additive, then None, then AlphaBlending over the same pixels"""
    quads = [wall(W, H, 60.0, -0.9, -0.8, 0.5, 0.6), wall(W, H, 45.0, -0.5, -0.9, 0.9, 0.4), wall(W, H, 75.0, -0.7, -0.5, 0.7, 0.9)]
    return cam_scene(W, H, [blended(draw(q[0], q[1], ids=[k]), m) for k, (q, m) in enumerate(zip(quads, ("additive", "none", "alpha")))], models=[IDENTITY] * 3,
                     mats=MATS, inst_materials=[0, 1, 2])


def deep_5(W=48, H=32):
    """five full-frame layers: one quad, five instances at distances 50, 40, 80, 60, 70 (all in front of the wall)"""
    q = wall(W, H, 1.0)
    models = [host.transform_matrix([0.0, 150.0 * (1.0 - d), 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [d, d, d, 1.0]) for d in (50.0, 40.0, 80.0, 60.0, 70.0)]
    return cam_scene(W, H, [blended(draw(q[0], q[1]), "alpha")], models=models, mats=MATS, inst_materials=[0, 1, 2, 0, 1])


def cutout_gltf(W=50, H=35):
    """a Standard quad, a glTF quad with ALPHA_CUTOUT over a bilinear alpha checker (its discarded fragments must not occupy a layer) and an emissive term, and
    an additive glTF quad on top"""
    quads = [wall(W, H, 70.0, -0.9, -0.9, 0.6, 0.7), wall(W, H, 55.0, -0.6, -0.7, 0.9, 0.9, uv=((0, 0), (2, 0), (2, 2), (0, 2))), wall(W, H, 45.0, -0.2, -0.6, 0.8, 0.3)]
    mats = [MATS[0], gltf_material(base=(0.4, 0.6, 0.9, 0.9), emissive=(0.6, 0.3, 0.1, 0), metallic=0.3, roughness=0.8, cutoff=0.4, samplers=(2, 1, 0, 0, 0)),
            gltf_material(base=(0.5, 0.7, 0.4, 0.3), emissive=(0.0, 0.2, 0.4, 0), metallic=0.2, roughness=0.6, samplers=(0, 1, 0, 0, 0))]
    draws = [blended(draw(quads[0][0], quads[0][1], ids=[0]), "alpha"), blended(cutout(gltf(draw(quads[1][0], quads[1][1], ids=[1]))), "alpha"),
             blended(gltf(draw(quads[2][0], quads[2][1], ids=[2])), "additive")]
    return cam_scene(W, H, draws, models=[IDENTITY] * 3, mats=mats, inst_materials=[0, 1, 2], textures=[WHITE, FLAT_NORMAL, checker(4)], srgb=[False] * 3)


def big_orders(W=48, H=32):
    """order_abc with primBase 2^31 - 3: the orders straddle 2^31, so the inverted key is exercised in its high bits"""
    s = order_abc(W, H)
    s["prim_base"] = 2 ** 31 - 3
    return s


def hostile_alpha(W=50, H=35):
    """vertex-colour alphas of 0, 1.5, NaN and Inf (one small quad each, material alpha 1) over an ordinary blended quad; the last two also under Additive"""
    back = wall(W, H, 70.0, -0.9, -0.9, 0.9, 0.9)
    v, t = [], []
    for k, a in enumerate((0.0, 1.5, np.nan, np.inf)):
        q = wall(W, H, 50.0, -0.8 + 0.4 * k, -0.5, -0.5 + 0.4 * k, 0.5, color=(0.8, 0.6, 0.4, a))
        t += [(4 * k + i0, 4 * k + i1, 4 * k + i2) for (i0, i1, i2) in q[1]]
        v += q[0]
    top = wall(W, H, 40.0, 0.0, -0.2, 0.8, 0.3, color=(0.5, 0.5, 0.5, np.inf))
    mats = [MATS[0], material(albedo=(1, 1, 1, 1), metallic=0.2, roughness=0.8)]
    return cam_scene(W, H, [blended(draw(back[0], back[1], ids=[0]), "alpha"), blended(draw(v, t, ids=[1]), "alpha"), blended(draw(top[0], top[1], ids=[1]), "additive")],
                     models=[IDENTITY] * 2, mats=mats, inst_materials=[0, 1])


def _per_pixel(stats, n):
    return int((stats["per_pixel"] == n).sum())


def _orders_at(layers, k):
    return set(int(x) for x in np.unique(layers[k]["last"])) - {0}


def _order_abc_reached(L, st, s, base=0):
    three = st["per_pixel"] == 3
    z = [L[k]["z"][three] for k in range(3)]
    return (len(L) == 3 and three.sum() > 30 and (z[1] > z[0]).all() and (z[2] < z[0]).all()          # B in front of A, C behind it
            and _orders_at(L, 0) >= {base + 1, base + 5} and all(int(x) > base + 8 for x in _orders_at(L, 2)))


CASES = {
    "order_abc": (order_abc, _order_abc_reached),
    "depth_edge": (depth_edge, lambda L, st, s: len(L) >= 2 and st["rejected"] > 100 and (L[0]["last"] == 1).sum() > 100 and (L[1]["last"] == 5).sum() > 100
                   and sum(int((l["last"] == 3).sum()) for l in L) < 10          # (a pixel of its snapped outline beside the prepass's triangle at the most)
                   and (L[0]["z"][L[0]["last"] == 1] == depth_attachment(s)[L[0]["last"] == 1]).all()),
    "self_overlap": (self_overlap, lambda L, st, s: len(L) >= 4 and _per_pixel(st, 2) > 50 and (L[1]["covered"] & (L[1]["last"] <= 24)).sum() > 50
                     and ((L[0]["last"] > 24) & (L[1]["last"] > 24) & (L[1]["last"] - L[0]["last"] == 4)).sum() > 50),
    "near_cut": (near_cut, lambda L, st, s: len(L) == 2 and (L[1]["last"] == 5).sum() > 10 and (L[1]["last"] == 6).sum() > 10),
    "mixed_modes": (mixed_modes, lambda L, st, s: len(L) == 3 and _per_pixel(st, 3) > 50 and set(np.unique(L[0]["blend"][L[0]["covered"]])) == {0, 1, 2}),
    "deep_5": (deep_5, lambda L, st, s: len(L) == 5 and (st["per_pixel"] == 5).all()),
    "cutout_gltf": (cutout_gltf, lambda L, st, s: st["discarded"] > 50 and len(L) == 3 and (L[1]["emissive"][..., :3].sum(-1) > 0).any()
                    and (L[0]["covered"] & (L[0]["last"] > 8)).sum() > 5),   # a pixel whose first fragment is the third draw's: the second draw's was discarded or absent
    "big_orders": (big_orders, lambda L, st, s: _order_abc_reached(L, st, s, 2 ** 31 - 3) and any(x < 2 ** 31 for x in _orders_at(L, 0))
                   and all(x > 2 ** 31 for x in _orders_at(L, 2))),
    "hostile_alpha": (hostile_alpha, lambda L, st, s: len(L) == 3 and all(f(L[1]["planes"][0][..., 3][L[1]["covered"]]).any()
                                                                         for f in (np.isnan, np.isinf, lambda a: a == 0, lambda a: a == 1.5))),
}


def all_scenes():
    return {name: build() for name, (build, _) in CASES.items()}


def target_of(s, seed=3):
    """what the passes before left in Main: finite, positive, every channel different"""
    return np.random.default_rng(seed).uniform(0, 1, (s["H"], s["W"], 4)).astype(f32)


def shaders(s, depth):
    """the shade of the opaque pass as the restatement's callables (planes, ao) -> radiance: the C oracle in fp32 and oracle_f64 in float64, both under the
    light lists culled against the depth attachment (rule 3: a transparent fragment sees its tile's list)"""
    from oracle import oracle, oracle_f64
    cam, l, W, H = s["cam"], s["lights"], s["W"], s["H"]
    og, oi, _ = oracle.light_cull(cam.frame, W, H, l, oracle.linearize_depth(cam.frame.cameraZNearZFar[0], depth))
    return (lambda planes, ao: oracle.shade(cam.frame, W, H, planes, l, og, oi, None)), (lambda planes, ao: oracle_f64.shade(bytes(cam.frame), W, H, planes, l, og, oi, None))


def chain_tolerance(layer_list, shade64, target, chain_error=0.0):
    """the shade's per-layer bound 1e-4 |f64| + 1e-7 max |f64| on every layer's radiance, propagated through the blend weights of the
    float64 chain, plus fp32's rounding of the blend itself (three roundings a channel and layer, 2^-23 of the operands each) -> float64 [n, W, 4].
    chain_error: an absolute allowance on top (the GPU test's 4 x the measured error of the fp32 restatement chain)."""
    import transparent_ref as tr
    out, tol = np.array(target, np.float64), np.zeros(np.shape(target), np.float64)
    eps = 2.0 ** -23
    with np.errstate(all="ignore"):
        for L in layer_list:
            rad = shade64(L["planes"], L["ao_out"])
            c, mode = L["covered"], L["blend"][..., None]
            src = tr.source(rad, L, np.float64)
            t_src = np.zeros_like(src)
            t_src[..., :3] = 1e-4 * np.abs(rad[..., :3]) + 1e-7 * np.abs(rad[c][:, :3]).max() + eps * np.abs(src[..., :3])
            a = src[..., 3:4]
            k = 1.0 - a
            alpha = np.abs(a) * t_src + np.abs(k) * tol + 3 * eps * (np.abs(src * a) + np.abs(out * k))
            new = np.where(mode == tr.NONE, t_src, np.where(mode == tr.ADDITIVE, t_src + tol + eps * (np.abs(src) + np.abs(out)), alpha))
            tol[c] = new[c]
            out[c] = tr.blend(L["blend"][c], src[c], out[c], np.float64)
    return np.nan_to_num(tol, nan=np.inf) + chain_error


# the worst |c32 - c64| of the fp32 restatement chain (C-oracle shade) over the cases' finite channels, as tests/test_transparent_cpu.py measures it (and holds the
# measurement to this figure within 1 %): what 4 x of the GPU test's end-to-end margin is taken from
CHAIN_ERROR = 4.53e-6   # the measurement (self_overlap, whose additive quads carry the largest radiance; every other case stays below 3e-7)
