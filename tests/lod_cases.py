"""The scenes of the mip-mapped texture tests (tests/test_lod_cpu.py, tests/test_lod_gpu.py): frames of at most 48 x 32, textures of 8 x 8, 5 x 3, 16 x 4,
17 x 9, 1 x 7, 1 x 1 and 64 x 64, built from the blocks of tests/surface_cases.py, tests/masked_cases.py and tests/gltf_cases.py.  A scene is the dict
tests/lod_ref.py describes: gltf_ref's, with `chains` (per texture the list of its levels) and `levels` (per texture the descriptor's field as written).
CASES maps a name to (builder, predicate(result of lod_ref.render, scene)): the predicate states what the case was built to reach."""
import numpy as np

import lod_ref
import surface_cases as sc
from gltf_cases import gltf, gltf_material
from masked_cases import cutout
from surface_cases import FLAT_NORMAL, draw, material, quad, scene, screen_projection, vertex

f32 = np.float32
EXTENTS = ((8, 8), (5, 3), (16, 4), (17, 9), (1, 7), (1, 1), (64, 64))   # width x height


def random_texture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def with_chains(s, levels=None):
    """every texture with the chain the restatement generates; levels: the descriptors' fields (default: the full count)"""
    s = dict(s)
    s["chains"] = [None if t.shape[0] == 0 or t.shape[1] == 0 else lod_ref.build_chain(t, g) for t, g in zip(s["textures"], s["srgb"])]
    s["levels"] = [1 if c is None else len(c) for c in s["chains"]] if levels is None else list(levels)
    return s


def constant_chain(w, h, colours):
    """a hand-made chain whose level l is the constant colour colours[l] (bytes, rgba)"""
    return [np.broadcast_to(np.array(colours[l], np.uint8), (lod_ref.level_extent(h, l), lod_ref.level_extent(w, l), 4)).copy()
            for l in range(lod_ref.full_levels(w, h))]


# bytes of 0 and 255 only: a fetched level is exactly 0.0 or 1.0 per channel, so a blend of two levels IS its weight, delta or 1 - delta, with no rounding of its own
LEVEL_COLOURS = [(255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (255, 255, 0, 255), (0, 255, 255, 255), (255, 0, 255, 255), (255, 255, 255, 255)]


def unorm(colour):
    return np.array(colour, f32) / f32(255)


def aligned_quad(texels_per_pixel_x, texels_per_pixel_y=None, W=24, H=16, size=64):
    """a screen-aligned quad over the whole frame whose texcoord advances texels_per_pixel texels of a size x size texture per pixel; the chain's level l is
    the constant LEVEL_COLOURS[l], UNORM; albedo 1, so P2.rgb is the fetched colour"""
    ty = texels_per_pixel_x if texels_per_pixel_y is None else texels_per_pixel_y
    u1, v1 = W * texels_per_pixel_x / size, H * ty / size
    v, t = quad(0.0, 0.0, float(W), float(H), uv=((0, 0), (u1, 0), (u1, v1), (0, v1)))
    s = scene(W, H, screen_projection(W, H), [draw(v, t)], textures=[np.zeros((size, size, 4), np.uint8), FLAT_NORMAL], srgb=[False, False],
              mats=[material(samplers=(0, 1, 1, 1))])
    s["chains"], s["levels"] = [constant_chain(size, size, LEVEL_COLOURS), None], [lod_ref.full_levels(size, size), 1]
    s["textures"][0] = s["chains"][0][0]
    return s


def receding_ground():
    """a plane rising from under the camera at the near plane to 30 units away: its rows cross every level boundary of the 64 x 64 albedo texture, from
    magnification to the 1 x 1 level; the other samplers are 16 x 4, 17 x 9 (the normal map, UNORM) and 5 x 3"""
    p = [(-1.5, -0.5, -1.0), (1.5, -0.5, -1.0), (36.0, 8.0, -30.0), (-36.0, 8.0, -30.0)]
    v = [vertex(q, (q[0] * 0.08, q[2] * 0.08), c) for q, c in zip(p, [(1, 0.9, 0.8, 1), (0.7, 1, 0.9, 1), (0.8, 0.8, 1, 1), (1, 1, 0.7, 0.9)])]
    tex = [random_texture(64, 64, 1), random_texture(16, 4, 2), random_texture(17, 9, 3), random_texture(5, 3, 4)]
    tex[2][..., 2] = 230
    return with_chains(scene(48, 32, sc.camera_projection(48, 32), [draw(v, [(0, 1, 2), (0, 2, 3)])], textures=tex, srgb=[True, True, False, True],
                             mats=[material(albedo=(0.9, 0.8, 0.7, 1), samplers=(0, 1, 2, 3))]))


def _every_level_of_descriptor_0(r, s):
    f = r["stats"]["fetched"]
    return all(f.get((0, l), 0) > 0 for l in range(7)) and len(r["stats"]["lambdas"]) > 0 and r["covered"].sum() > 300


def near_cut():
    """triangles with one and with two vertices beyond the near plane under minifying texcoords: both parts of the first own pixels"""
    col = [(1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 1, 1)]
    uvs = [(0, 0), (7, 0), (0, 9)]
    tris = [[(-1.5, -0.5, -3.0), (-0.2, -0.7, -0.4), (-0.9, 0.8, -2.5)], [(0.3, -0.6, -0.5), (1.6, -0.4, -0.6), (1.0, 0.9, -3.5)]]
    v = [vertex(p, uvs[k], col[k]) for tri in tris for k, p in enumerate(tri)]
    tex = [random_texture(8, 8, 5), FLAT_NORMAL, random_texture(1, 7, 6)]
    return with_chains(scene(48, 32, sc.camera_projection(48, 32), [draw(v, [(0, 1, 2), (3, 5, 4)])], textures=tex, srgb=[True, False, False],
                             mats=[material(samplers=(0, 2, 1, 2))]))


def _both_parts(r, s):
    low = (r["keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    parts = {int(x) for x in np.unique(low[low > 0] - 1)}
    return r["stats"]["cut_two"] == 1 and r["stats"]["cut_one"] == 1 and {0, 1, 2} <= parts and any(l > 0 for (_, l) in r["stats"]["fetched"])


def one_pixel_triangles():
    """triangles that cover one pixel centre each: the quad's other centres lie outside the triangle"""
    v, t = [], []
    for k, (cx, cy) in enumerate([(3.5, 2.5), (10.5, 7.5), (20.5, 4.5), (31.5, 12.5), (14.5, 15.5), (36.5, 20.5)]):
        du = 0.3 * (k + 1)
        v += [vertex((cx - 0.4, cy - 0.3, 0.5), (0, 0)), vertex((cx + 0.45, cy - 0.2, 0.5), (du, 0.1)), vertex((cx, cy + 0.45, 0.5), (0.2, du))]
        t.append((3 * k, 3 * k + 1, 3 * k + 2))
    tex = [random_texture(8, 8, 7), FLAT_NORMAL, random_texture(17, 9, 8)]
    return with_chains(scene(37, 21, screen_projection(37, 21), [draw(v, t)], textures=tex, srgb=[False, False, True], mats=[material(samplers=(0, 2, 1, 2))]))


def _helpers_outside(r, s):
    return r["covered"].sum() == 6 and r["stats"]["helpers_outside"] >= 6 and any(l > 0 for (_, l) in r["stats"]["fetched"])


def horizon_next_to_a_covered_pixel():
    """a triangle whose plane's horizon (s == 0) is the row of pixel centres just above its top edge: the column mates of row 5 are evaluated ON it -- s is
    exactly 0 in the symmetric column (uv NaN) and a rounding residue of either sign elsewhere (uv huge)"""
    W, H = 48, 32
    P = np.zeros(16, f32)
    P[0], P[5], P[11], P[14] = 1.0, 1.0, -1.0, 1.0                       # clip = (x, y, 1, -z): depth 1 / w
    horizon = 4.5

    def at(xf, yf):
        w = 1.0 / ((yf - horizon) / (H / 2))                            # 1 / w falls to 0 on the horizon row
        return ((2 * xf / W - 1) * w, (1 - 2 * yf / H) * w, -w)
    v = [vertex(at(9.5, 5.0), (0.0, 0.0)), vertex(at(21.5, 5.0), (3.0, 0.0)), vertex(at(15.5, 12.5), (1.5, 2.0))]
    tex = [random_texture(8, 8, 9), FLAT_NORMAL]
    return with_chains(scene(W, H, P, [draw(v, [(0, 1, 2)])], textures=tex, srgb=[True, False], mats=[material(samplers=(0, 0, 1, 0))]))


def _reached_the_horizon(r, s):
    return r["covered"][5, 15] and r["stats"]["nonfinite_derivs"] >= 1 and r["covered"].sum() > 20


def odd_frame():
    """37 x 21: the row mate of the last column and the column mate of the last row lie outside the frame"""
    W, H = 37, 21
    v, t = quad(0.0, 0.0, float(W), float(H), uv=((0, 0), (5.5, 0), (5.5, 4.25), (0, 4.25)))
    tex = [random_texture(16, 4, 10), FLAT_NORMAL, random_texture(5, 3, 11)]
    return with_chains(scene(W, H, screen_projection(W, H), [draw(v, t)], textures=tex, srgb=[True, False, False], mats=[material(samplers=(0, 2, 1, 2))]))


def _helpers_off_frame(r, s):
    return r["covered"].all() and r["stats"]["helpers_off_frame"] == 37 + 21


def anisotropic():
    """8 texels per pixel in u against 1 in v: the larger axis decides, level 3"""
    return aligned_quad(8, 1)


def _level_3(r, s):
    f = r["stats"]["fetched"]
    return set(l for (d, l) in f if d == 0) <= {2, 3, 4} and f.get((0, 3), 0) == r["covered"].sum()


def levels_field_0_1_99():
    """three descriptors over the same 8 x 8 image whose `levels` fields are 0, 1 and 99, four texels per pixel: one level, one level, the full four"""
    W, H = 36, 16
    img = random_texture(8, 8, 12)
    v, t = [], []
    for k in range(3):
        q, _ = quad(12.0 * k, 0.0, 12.0 * k + 12.0, float(H), uv=((0, 0), (6, 0), (6, 8), (0, 8)))
        v += q
        t += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
    draws = [draw(v[4 * k: 4 * k + 4], [(0, 1, 2), (0, 2, 3)], first_instance=k, num_drawn=1) for k in range(3)]
    s = scene(W, H, screen_projection(W, H), draws, models=[sc.IDENTITY] * 3, textures=[img, img, img, FLAT_NORMAL], srgb=[True, True, True, False],
              mats=[material(samplers=(k, k, 3, k)) for k in range(3)], inst_materials=[0, 1, 2])
    return with_chains(s, levels=[0, 1, 99, 1])


def _fields_clamped(r, s):
    f = r["stats"]["fetched"]
    return {l for (d, l) in f if d == 0} == {0} and {l for (d, l) in f if d == 1} == {0} and max(l for (d, l) in f if d == 2) >= 2


def mixed_pass():
    """a Standard and a glTF draw in one pass over chains, the glTF one with orm, occlusion and emissive textures"""
    W, H = 48, 32
    a, t = quad(0.0, 0.0, 30.0, float(H), z=0.4, uv=((0, 0), (9, 0), (9, 7), (0, 7)))
    b, _ = quad(18.0, 4.0, float(W), 28.0, z=0.6, uv=((0, 0), (2.5, 0), (2.5, 6), (0, 6)))
    tex = [random_texture(8, 8, 13), FLAT_NORMAL, random_texture(16, 4, 14), random_texture(17, 9, 15), random_texture(1, 7, 16), random_texture(1, 1, 17)]
    mats = [material(albedo=(0.9, 0.8, 0.7, 1), samplers=(0, 2, 1, 4)),
            gltf_material(base=(0.8, 0.9, 1.0, 1.0), emissive=(0.5, 0.4, 0.3, 0), metallic=0.6, roughness=0.7, normal_scale=0.8, samplers=(3, 1, 2, 4, 0))]
    s = scene(W, H, screen_projection(W, H), [draw(a, t, first_instance=0, num_drawn=1), gltf(draw(b, t, first_instance=1, num_drawn=1))],
              models=[sc.IDENTITY] * 2, textures=tex, srgb=[True, False, True, True, False, True], mats=mats, inst_materials=[0, 1])
    s["ao_in"] = np.random.default_rng(18).uniform(0.2, 1.0, (H, W)).astype(f32)
    return with_chains(s)


def _both_shaders(r, s):
    c = r["covered"]
    return (r["gltf"] & c).sum() > 100 and (~r["gltf"] & c).sum() > 100 and (r["emissive"][r["gltf"]][:, :3] > 0).any() and \
        sum(1 for (d, l) in r["stats"]["fetched"] if l > 0) >= 4


def alpha_chain(w, h, alphas, seed):
    """a hand-made chain whose level l has the constant alpha alphas[l] over random colours"""
    chain = [random_texture(lod_ref.level_extent(w, l), lod_ref.level_extent(h, l), seed + l) for l in range(lod_ref.full_levels(w, h))]
    for l, c in enumerate(chain):
        c[..., 3] = alphas[l]
    return chain


def cutout_per_level():
    """cutout grounds, Standard (threshold 0.5) and glTF (alphaCutoff 0.3), whose albedo chains hold another alpha in every level: which rows survive is
    decided by the level of detail, and the blend of two levels crosses the threshold inside a row band"""
    W, H = 48, 32
    alphas = [255, 40, 230, 20, 250, 90, 200]
    chain_a, chain_b = alpha_chain(64, 64, alphas, 20), alpha_chain(8, 8, alphas[3:], 40)
    far, tint = -120.0, [(1, 0.9, 0.8, 1), (0.7, 1, 0.9, 1), (0.8, 0.8, 1, 1), (1, 1, 0.7, 0.9)]
    half = lambda p, scale: [vertex(q, (q[0] * scale, q[2] * scale), c) for q, c in zip(p, tint)]
    lv = half([(-1.5, -0.5, -1.0), (0.0, -0.5, -1.0), (0.0, -0.4, far), (-60.0, -0.4, far)], 0.5)     # the left half of the view and the right half, one draw each
    rv = half([(0.0, -0.5, -1.0), (1.5, -0.5, -1.0), (60.0, -0.4, far), (0.0, -0.4, far)], 1.5)
    tris = [(0, 1, 2), (0, 2, 3)]
    mats = [material(albedo=(1, 1, 1, 1), samplers=(0, 2, 1, 2)), gltf_material(base=(1, 1, 1, 0.9), cutoff=0.3, samplers=(3, 1, 2, 2, 2))]
    s = scene(W, H, sc.camera_projection(W, H), [cutout(draw(lv, tris, first_instance=0, num_drawn=1)),
                                                 cutout(gltf(draw(rv, tris, first_instance=1, num_drawn=1)))],
              models=[sc.IDENTITY] * 2, textures=[chain_a[0], FLAT_NORMAL, sc.WHITE, chain_b[0]], srgb=[True, False, False, True], mats=mats, inst_materials=[0, 1])
    s["chains"], s["levels"] = [chain_a, None, None, chain_b], [7, 1, 1, 4]
    return s


def _discard_follows_the_level(r, s):
    st = r["stats"]
    own = r["cutout"] & r["covered"]
    return st["discarded"] > 50 and own.sum() > 50 and (r["gltf"] & own).sum() > 10 and (~r["gltf"] & own).sum() > 10 and \
        len({l for (d, l) in st["fetched"] if d == 0}) >= 4


CASES = {
    "receding_ground": (receding_ground, _every_level_of_descriptor_0),
    "near_cut": (near_cut, _both_parts),
    "one_pixel_triangles": (one_pixel_triangles, _helpers_outside),
    "horizon_next_to_a_covered_pixel": (horizon_next_to_a_covered_pixel, _reached_the_horizon),
    "odd_frame": (odd_frame, _helpers_off_frame),
    "anisotropic": (anisotropic, _level_3),
    "levels_field_0_1_99": (levels_field_0_1_99, _fields_clamped),
    "mixed_pass": (mixed_pass, _both_shaders),
    "cutout_per_level": (cutout_per_level, _discard_follows_the_level),
}
BAND_CASES = ("receding_ground", "cutout_per_level", "mixed_pass")   # 48 x 32: two tile rows


def all_scenes():
    return {name: build() for name, (build, _) in CASES.items()}


def one_level(s):
    """the scene with every descriptor at one level"""
    s = dict(s)
    s.pop("chains", None)
    s.pop("levels", None)
    return s
