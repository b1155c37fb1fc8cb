"""The scenes of the Masked-queue tests (tests/test_masked_cpu.py, tests/test_masked_gpu.py): small frames, 40 x 24 to 96 x 72, built from the blocks of
tests/surface_cases.py.  A scene is the dict tests/surface_ref.py describes; a draw that carries alpha_cutout=True is a draw of the ALPHA_CUTOUT
permutation.  CASES maps a name to (builder, predicate(result of masked_ref.render, scene)): the predicate states what the case was built to reach, over the
restatement's counts, so that a case cannot silently stop reaching its branch."""
import numpy as np

import masked_ref
import surface_cases as sc
from surface_cases import FLAT_NORMAL, IDENTITY, WHITE, draw, material, quad, scene, screen_projection, translation, vertex

f32 = np.float32
LOW = np.uint64(0xFFFFFFFF)
NO_TEXELS = np.zeros((0, 0, 4), np.uint8)


def cutout(d, on=True):
    d = dict(d)
    d["alpha_cutout"] = on
    return d


def alpha_texture(alpha):
    """white texels with the given alpha bytes [h, w]"""
    a = np.asarray(alpha, np.uint8)
    t = np.full(a.shape + (4,), 255, np.uint8)
    t[..., 3] = a
    return t


def checker(n=4):
    return alpha_texture(((np.arange(n)[:, None] + np.arange(n)[None, :]) & 1) * 255)


def orders(r):
    return set(int(x) for x in np.unique(r["keys"] & LOW))


# ---- the threshold --------------------------------------------------------------------------------------------------------------------------------
def threshold_bytes():
    """1 x 1 textures with alpha byte 127 (127 / 255 < 0.5: every fragment discarded) and 128 (kept)"""
    v, t = quad(2.5, 3.5, 14.5, 19.5)
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, t, ids=[0, 1]))], models=[IDENTITY, translation(20.0, 0.0, 0.0)],
                 textures=[WHITE, FLAT_NORMAL, alpha_texture([[127]]), alpha_texture([[128]])],
                 mats=[material(samplers=(2, 0, 1, 0)), material(samplers=(3, 0, 1, 0))], inst_materials=[0, 1])


def threshold_exact():
    """material alpha 0.5 x byte 255 x colour 1 is exactly 0.5 and kept; nextafter(0.5, 0) is discarded.  The quads are 16 x 16 pixels with their corners on
    pixel centres under the orthographic matrix (w = 1), so every l_k is a multiple of 1 / 16, s is exactly 1 and the colour alpha is exactly 1"""
    v, t = quad(2.5, 3.5, 18.5, 19.5)
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, t, ids=[0, 1]))], models=[IDENTITY, translation(19.0, 0.0, 0.0)],
                 mats=[material(albedo=(1, 1, 1, 0.5)), material(albedo=(1, 1, 1, np.nextafter(f32(0.5), f32(0))))], inst_materials=[0, 1])


def bilinear_ramp_srgb():
    """a 2 x 1 sRGB texture with alpha 0 and 255 under u = 0.25 .. 0.75 over 32 pixel columns: alpha = k / 32 exactly at column k, so 16 of the 32 columns are
    kept and the one at exactly 0.5 among them.  Were alpha sRGB-decoded, the ramp would cross 0.5 near column 24."""
    v, t = quad(4.5, 3.5, 36.5, 19.5, uv=((0.25, 0.5), (0.75, 0.5), (0.75, 0.5), (0.25, 0.5)))
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, t))], textures=[alpha_texture([[0, 255]]), FLAT_NORMAL], srgb=[True, False])


# ---- interpolation --------------------------------------------------------------------------------------------------------------------------------
def colour_alpha_oblique():
    """vertex colour alpha 1 -> 0 along a ground quad seen at a grazing angle (clip w from 1 to 50): under a material alpha of 0.52 the perspective-correct
    alpha 0.52 (1 - t) crosses 0.5 at t = 1 / 26 of the way into the world, in the middle of the screen; the screen-linear one a twenty-sixth up the quad"""
    p = [(-1.0, -0.5, -1.0), (1.0, -0.5, -1.0), (40.0, -0.4, -50.0), (-40.0, -0.4, -50.0)]
    v = [vertex(q, (q[0] * 0.25, q[2] * 0.25), (1, 1, 1, a)) for q, a in zip(p, (1.0, 1.0, 0.0, 0.0))]
    return scene(72, 40, sc.camera_projection(72, 40), [cutout(draw(v, [(0, 1, 2), (0, 2, 3)]))], mats=[material(albedo=(1, 1, 1, 0.52))])


def cut_vertices():
    """surface_cases.near_plane (a triangle the near plane cuts in one and triangles it cuts in two) with the colour alpha varying from vertex to vertex"""
    s = sc.near_plane()
    d = s["draws"][0]
    d["vertices"][:, 17] = np.tile(np.array([0.15, 0.95, 0.6], f32), 3)
    s["draws"] = [cutout(d)]
    return s


def nan_inf_negative_alpha():
    """material alpha NaN and +inf survive, a negative alpha is discarded"""
    v, t = quad(1.5, 2.5, 11.5, 20.5)
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, t, ids=[0, 1, 2]))], models=[IDENTITY, translation(13.0, 0.0, 0.0), translation(26.0, 0.0, 0.0)],
                 mats=[material(albedo=(1, 1, 1, np.nan)), material(albedo=(1, 1, 1, np.inf)), material(albedo=(1, 1, 1, -3.0))], inst_materials=[0, 1, 2])


# ---- depth test and ordering ----------------------------------------------------------------------------------------------------------------------
def checker_over_opaque():
    """a 4 x 4 0 / 255 alpha checker quad over a farther opaque quad drawn without the flag: the holes hold the opaque quad's order"""
    far, near = quad(1.3, 1.2, 38.6, 22.7, z=0.3), quad(5.2, 3.1, 33.7, 20.4, z=0.7, uv=((0, 0), (1, 0), (1, 1), (0, 1)))
    return scene(40, 24, screen_projection(40, 24), [draw(far[0], far[1], ids=[0]), cutout(draw(near[0], near[1], ids=[1]))], models=[IDENTITY, IDENTITY],
                 textures=[WHITE, FLAT_NORMAL, checker()], mats=[material(albedo=(0.2, 0.4, 0.8, 1)), material(samplers=(2, 0, 1, 0))], inst_materials=[0, 1])


def discarded_in_front():
    """a fully transparent nearer triangle drawn last leaves every key alone"""
    s = sc.multiple_draws()
    tri = [vertex((2.1, 1.3, 0.95)), vertex((38.2, 2.2, 0.95)), vertex((19.3, 23.1, 0.95))]
    s["textures"] = s["textures"] + [alpha_texture([[0]])]
    s["srgb"] = s["srgb"] + [False]
    s["materials"] = np.concatenate([s["materials"], material(samplers=(2, 0, 1, 0))])
    s["instances"] = sc.instances([IDENTITY, translation(6.0, 3.0, 0.1), translation(-3.0, 2.0, 0.2), IDENTITY], [0, 1, 2, 3])
    s["draws"] = s["draws"] + [cutout(draw(tri, [(0, 1, 2)], ids=[3]))]
    return s


def without_last_draw(s):
    s = dict(s)
    s["draws"] = s["draws"][:-1]
    return s


def tie_later_discarded():
    """two coincident triangles (two instances of one draw); the later one's fragments are discarded on half the area (a 2 x 1 alpha 255 | 0 texture): the
    earlier order wins there and the later elsewhere"""
    v = [vertex((4.2, 3.1, 0.4), (0.0, 0.5)), vertex((33.7, 5.3, 0.6), (1.0, 0.5)), vertex((17.9, 21.2, 0.7), (0.5, 0.5))]
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, [(0, 1, 2)], ids=[0, 1]))], models=[IDENTITY, IDENTITY],
                 textures=[WHITE, FLAT_NORMAL, alpha_texture([[255, 0]])], mats=[material(), material(albedo=(0.5, 0.25, 0.125, 1), samplers=(2, 0, 1, 0))],
                 inst_materials=[0, 1])


def large_checker_two_superblocks():
    """96 x 72 (two 64-texel superblocks each way) under a triangle larger than the frame with the checker: the wave path"""
    big = [vertex((-150.0, -100.0, 0.2), (0, 0), (1, 0, 0, 1)), vertex((350.0, -75.0, 0.4), (6, 0), (0, 1, 0, 1)), vertex((50.0, 300.0, 0.3), (0, 6), (0, 0, 1, 1))]
    return scene(96, 72, screen_projection(96, 72), [cutout(draw(big, [(0, 1, 2)]))], textures=[checker(), FLAT_NORMAL])


def flag_absent():
    """no draw carries the flag: through either entry point the keys are surface_ref's"""
    return sc.multiple_draws()


# ---- look-ups -------------------------------------------------------------------------------------------------------------------------------------
def per_instance_materials():
    """one draw, instance indirection, five materials with five albedo samplers in one wave"""
    v, t = quad(0.0, 0.0, 11.3, 9.1, z=0.5, uv=((0, 0), (2, 0), (2, 2), (0, 2)))
    models = [translation(5.5 * k, 2.7 * k, 0.01 * k) for k in range(6)]
    tex = [WHITE, FLAT_NORMAL, checker(2), checker(4), alpha_texture([[255, 0, 255]]), alpha_texture([[0], [255]]), alpha_texture([[200, 100], [60, 255]])]
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, t, ids=[4, 1, 1, 3, 0, 2, 5]))], models=models, textures=tex,
                 mats=[material(albedo=(k / 6 + 0.1, 1 - k / 6, 0.5, 1), samplers=(2 + k, 0, 1, 0)) for k in range(5)], inst_materials=[0, 1, 2, 3, 4, 0])


def no_texels_and_beyond_table():
    """a materialInstance beyond numMaterials reads material 0, a sampler index beyond numTextures reads descriptor 0 (both kept: descriptor 0 is opaque
    white), a descriptor without texels samples 0 (everything discarded)"""
    v, t = quad(1.5, 2.5, 11.5, 20.5)
    return scene(40, 24, screen_projection(40, 24), [cutout(draw(v, t, ids=[0, 1, 2]))], models=[IDENTITY, translation(13.0, 0.0, 0.0), translation(26.0, 0.0, 0.0)],
                 textures=[WHITE, FLAT_NORMAL, NO_TEXELS], mats=[material(), material(samplers=(7, 0, 1, 0)), material(samplers=(2, 0, 1, 0))],
                 inst_materials=[9, 1, 2])


# ---- random ---------------------------------------------------------------------------------------------------------------------------------------
NUM_SOUPS = 20


def masked_soup(seed):
    """surface_cases.random_soup with alpha textures whose bytes are 0 or 255 (steep ramps: few fragments near the threshold), material alphas of 0.8 .. 1.6,
    colour alphas of 0.7 .. 1 and the flag on the second draw or on both"""
    s = sc.random_soup(seed)
    rng = np.random.default_rng(5000 + seed)
    for k, t in enumerate(s["textures"]):
        t = t.copy()
        t[..., 3] = rng.integers(0, 2, t.shape[:2]) * 255
        s["textures"][k] = t
    s["materials"]["albedo"][:, 3] = rng.uniform(0.8, 1.6, len(s["materials"])).astype(f32)
    for d in s["draws"]:
        d["vertices"][:, 17] = rng.uniform(0.7, 1.0, len(d["vertices"])).astype(f32)
    s["draws"] = [cutout(s["draws"][0], bool(seed & 2)), cutout(s["draws"][1])]
    return s


def _inside(r, x0, x1):
    return r["covered"][:, x0:x1]


CASES = {
    "threshold_bytes": (threshold_bytes, lambda r, s: r["stats"]["discarded"] == 12 * 16 and r["covered"].sum() == 12 * 16 and not _inside(r, 0, 20).any()),
    "threshold_exact": (threshold_exact, lambda r, s: r["stats"]["exactly_half"] == 256 and r["stats"]["discarded"] == 256 and r["covered"].sum() == 256
                        and not _inside(r, 21, 40).any()),
    "bilinear_ramp_srgb": (bilinear_ramp_srgb, lambda r, s: r["covered"].sum() == 16 * 16 and r["stats"]["exactly_half"] == 16 and r["covered"][:, 20:36].sum() == 256
                           and r["stats"]["taps"]["srgb"] > 0),
    "colour_alpha_oblique": (colour_alpha_oblique, lambda r, s: r["stats"]["discarded"] > 50 and r["covered"].sum() > 50
                             and (masked_ref.render(s, perspective=False)["covered"] != r["covered"]).sum() > 50),
    "cut_vertices": (cut_vertices, lambda r, s: r["stats"]["cut_one"] >= 1 and r["stats"]["cut_two"] >= 2 and r["stats"]["discarded"] > 20
                     and any(x and x % 2 == 0 for x in orders(r))),   # (an even low word: the second half of a triangle cut in two)
    "nan_inf_negative_alpha": (nan_inf_negative_alpha, lambda r, s: r["stats"]["nan_alpha"] == 180 and r["covered"].sum() == 360 and not _inside(r, 27, 40).any()
                               and np.isinf(r["planes"][0][..., 3]).sum() == 180),
    "checker_over_opaque": (checker_over_opaque, lambda r, s: r["stats"]["discarded"] > 100 and (r["cutout"].sum() > 100)
                            and ((r["keys"][4:20, 6:33] & LOW) <= np.uint64(2)).sum() > 100),
    "discarded_in_front": (discarded_in_front, lambda r, s: r["stats"]["discarded"] > 200 and max(orders(r)) <= 16
                           and np.array_equal(r["keys"], masked_ref.render(without_last_draw(s))["keys"])),
    "tie_later_discarded": (tie_later_discarded, lambda r, s: r["stats"]["discarded_at_tie"] > 50 and orders(r) == {0, 1, 3}),
    "large_checker_two_superblocks": (large_checker_two_superblocks, lambda r, s: r["stats"]["large"] >= 1 and r["stats"]["discarded"] > 1000 and r["covered"].sum() > 1000
                                      and r["covered"][:, :64].any() and r["covered"][:, 64:].any() and r["covered"][64:].any()),
    "flag_absent": (flag_absent, lambda r, s: r["stats"]["tested"] == 0 and r["covered"].any()),
    "per_instance_materials": (per_instance_materials, lambda r, s: len(r["stats"]["materials"]) == 5 and r["stats"]["discarded"] > 50),
    "no_texels_and_beyond_table": (no_texels_and_beyond_table, lambda r, s: r["stats"]["beyond_table"] > 0 and r["stats"]["discarded"] == 180 and r["covered"].sum() == 360
                                   and not _inside(r, 27, 40).any()),
}
EXACT_THRESHOLD_CASES = ("threshold_bytes", "threshold_exact", "bilinear_ramp_srgb")
CULL_BACK_CASES = ("checker_over_opaque", "cut_vertices", "tie_later_discarded")
BAND_CASES = ("colour_alpha_oblique", "cut_vertices", "large_checker_two_superblocks")   # 72 x 40 and 96 x 72: more than one tile row
GOLDEN_CASE = "checker_over_opaque"


def all_scenes():
    """name -> scene, the cases and the soups"""
    out = {name: build() for name, (build, _) in CASES.items()}
    out.update({f"masked_soup_{seed}": masked_soup(seed) for seed in range(NUM_SOUPS)})
    return out


def opaque_prepass(s):
    """the Opaque depth prepass: the project's oracle over the draws WITHOUT the flag"""
    o = dict(s)
    o["draws"] = [d for d in s["draws"] if not d.get("alpha_cutout", False)]
    return sc.prepass_depth(o)


def full_prepass(s):
    """DepthPrepass Opaque, then Masked: what a RenderScene pass of the scene starts from"""
    return masked_ref.masked_prepass_depth(s, opaque_prepass(s))
