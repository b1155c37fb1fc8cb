"""The scenes of the glTF-material tests (tests/test_gltf_cpu.py, tests/test_gltf_gpu.py): small frames, 40 x 24 to 96 x 72, built from the blocks of
tests/surface_cases.py and tests/masked_cases.py.  A scene is the dict tests/gltf_ref.py describes: a draw may carry gltf=True and alpha_cutout=True, the scene may
carry ao_in.  The material table is ONE array of 80-byte slots; gltf_material() builds a slot as the glTF record.  CASES maps a name to
(builder, predicate(result of gltf_ref.render, scene)): the predicate states what the case was built to reach, so that it cannot silently stop reaching it."""
import numpy as np

import gltf_ref
import masked_cases as mc
import masked_ref
import surface_cases as sc
from masked_cases import LOW, NO_TEXELS, alpha_texture, checker, cutout, orders
from sailor_amd import _lib, host
from surface_cases import FLAT_NORMAL, IDENTITY, WHITE, draw, material, quad, scene, screen_projection, translation, vertex

f32 = np.float32
STANDARD, GLTF = np.dtype(_lib.MATERIAL_DTYPE), np.dtype(_lib.GLTF_MATERIAL_DTYPE)


def gltf(d, on=True):
    d = dict(d)
    d["gltf"] = on
    return d


def gltf_material(base=(1, 1, 1, 1), emissive=(0, 0, 0, 0), metallic=1.0, roughness=1.0, normal_scale=1.0, cutoff=0.5, samplers=(0, 1, 0, 0, 0), strength=1.0):
    """samplers = (baseColor, normal, orm, occlusion, emissive) -> one slot of the table (a MATERIAL_DTYPE record holding the glTF record's bytes)"""
    m = np.zeros(1, GLTF)
    m["baseColorFactor"], m["emissiveFactor"], m["metallicFactor"], m["roughnessFactor"] = base, emissive, metallic, roughness
    m["occlusionStrength"], m["normalScale"], m["alphaCutoff"] = strength, normal_scale, cutoff
    m["baseColorSampler"], m["normalSampler"], m["ormSampler"], m["occlusionSampler"], m["emissiveSampler"] = samplers
    return m.view(STANDARD)


def as_gltf(s, cutoff=0.5):
    """the scene with every draw flagged glTF and every material slot rewritten as the equivalent glTF record: baseColor = albedo through the same sampler,
    metallic / roughness through the metalness sampler's .b / .g, occlusion and emissive through descriptor 0"""
    s = dict(s)
    old = s["materials"]
    s["materials"] = np.concatenate([gltf_material(base=m["albedo"], metallic=m["metallic"], roughness=m["roughness"], cutoff=cutoff,
                                                   samplers=(m["albedoSampler"], m["normalSampler"], m["metalnessSampler"], 0, 0)) for m in old])
    s["draws"] = [gltf(d) for d in s["draws"]]
    return s


def tilted_normal_map(seed=5):
    rng = np.random.default_rng(seed)
    nm = rng.integers(60, 200, (4, 4, 4), dtype=np.uint8)
    nm[..., 2] = 230
    return nm


def rgb_texture(w, h, seed):
    """r, g and b differ in every texel (and from texel to texel)"""
    t = sc.distinct_texture(w, h, seed)
    t[..., 1], t[..., 2] = t[..., 0] + np.uint8(85), t[..., 0] + np.uint8(170)   # (modulo 256)
    return t


def _basis_quad(half=1.0):
    p = [(-half, -half, 0.0), (half, -half, 0.0), (half, half, 0.0), (-half, half, 0.0)]
    return [vertex(q, (0.5 * q[0] / half + 0.5, 0.5 * q[1] / half + 0.5), normal=(0.1, 0.2, 0.97), tangent=(0.98, 0.0, -0.1), bitangent=(0.0, 0.97, -0.2)) for q in p]


# ---- the normal matrix ------------------------------------------------------------------------------------------------------------------------------
NORMAL_MODELS = dict(scaled_rotated=([-4.5, 1.2, -6.0, 1.0], [0.18, 0.37, 0.09, 0.907], [1.5, 0.6, 1.0, 1.0]),
                     mirrored=([-1.5, -1.0, -6.0, 1.0], [-0.3, 0.1, 0.2, 0.927], [-1.2, 1.4, 0.7, 1.0]),
                     anisotropic=([1.7, 1.3, -6.0, 1.0], [0.1, -0.2, 0.05, 0.973], [1.3, 1.1, 400.0, 1.0]),
                     singular=([4.7, -0.9, -6.0, 1.0], [0.0, 0.0, 0.2588, 0.9659], [1.2, 1.3, 0.0, 1.0]))


def normal_matrix_models():
    """one quad under four models: non-uniform scale plus rotation, a mirrored one (negative determinant), a strongly anisotropic one, a singular one (z scale 0:
    the flat quad still rasterises, its normals are not finite)"""
    models = [host.transform_matrix(*trs) for trs in NORMAL_MODELS.values()]
    return scene(72, 40, sc.camera_projection(72, 40), [gltf(draw(_basis_quad(), [(0, 1, 2), (0, 2, 3)], cull_back=False))], models=models,
                 textures=[WHITE, tilted_normal_map()], mats=[gltf_material()])


def _det3(m):
    return float(np.linalg.det(np.asarray(m, np.float64).reshape(4, 4).T[:3, :3]))


def _normal_matrix_reached(r, s):
    owner = (r["keys"] & LOW).astype(np.int64)
    per = [((owner == 4 * k + 1) | (owner == 4 * k + 3)) for k in range(4)]   # instance k: orders 4k + (0, 2)
    n = r["planes"][1][..., :3]
    mutant = gltf_ref.render(s, standard_basis=True)["planes"][1][..., :3]
    models = s["instances"]["model"]
    return (all(p.sum() > 20 for p in per) and np.isfinite(n[per[0] | per[1] | per[2]]).all() and not np.isfinite(n[per[3]]).any()
            and _det3(models[1]) < 0 and _det3(models[3]) == 0
            and all((np.abs(n[p] - mutant[p]).max(axis=-1) > 1e-2).mean() > 0.9 for p in per[:3]))


def normal_matrix_near_plane():
    """surface_cases.near_plane (a triangle cut in one, triangles cut in two) as a glTF draw under a model that scales x and y apart and rotates about z (the
    vertices' z, and with it every cut, stays), each vertex with its own tangent frame"""
    s = sc.near_plane()
    d = s["draws"][0]
    rng = np.random.default_rng(3)
    d["vertices"][:, 5:14] = rng.uniform(-1, 1, (len(d["vertices"]), 9)).astype(f32)
    s["draws"] = [gltf(d)]
    s["instances"] = sc.instances([host.transform_matrix([0.1, 0.05, 0.0, 1.0], [0.0, 0.0, 0.1305, 0.9914], [1.3, 0.7, 1.0, 1.0])])
    s["textures"], s["srgb"] = [WHITE, tilted_normal_map()], [False, False]
    s["materials"] = gltf_material()
    return s


# ---- the fetches ------------------------------------------------------------------------------------------------------------------------------------
def orm_channels():
    """metallic from .b and roughness from .g of ONE texture whose r, g, b differ in every texel; the same image behind a UNORM and an sRGB descriptor"""
    v, t = quad(1.5, 2.5, 18.5, 21.5, uv=((0.1, 0.2), (1.7, 0.2), (1.7, 1.4), (0.1, 1.4)))
    img = rgb_texture(4, 3, 21)
    return scene(40, 24, screen_projection(40, 24), [gltf(draw(v, t, ids=[0, 1]))], models=[IDENTITY, translation(19.0, 0.0, 0.0)],
                 textures=[WHITE, FLAT_NORMAL, img, img.copy()], srgb=[False, False, False, True],
                 mats=[gltf_material(metallic=0.9, roughness=0.8, samplers=(0, 1, 2, 0, 0)), gltf_material(metallic=0.9, roughness=0.8, samplers=(0, 1, 3, 0, 0))],
                 inst_materials=[0, 1])


def _orm_reached(r, s):
    def variant(f):
        q = dict(s)
        q["textures"] = [t if k < 2 else f(t) for k, t in enumerate(s["textures"])]
        return gltf_ref.render(q)["planes"]
    g = r["gltf"]
    red = variant(lambda t: t[..., [0, 0, 0, 3]])       # what reading .r for both would give
    swap = variant(lambda t: t[..., [0, 2, 1, 3]])      # .g and .b swapped
    met, rough = r["planes"][2][..., 3], r["planes"][1][..., 3]
    return (g.sum() == 2 * 17 * 19 and r["stats"]["taps"]["srgb"] > 0 and (met[g] != red[2][..., 3][g]).mean() > 0.9 and (rough[g] != red[1][..., 3][g]).mean() > 0.9
            and (met[g] != swap[2][..., 3][g]).mean() > 0.9 and (met[:, :19][g[:, :19]] != met[:, 19:38][g[:, 19:38]]).mean() > 0.9)


OCC = f32(128) / f32(255)   # the occlusion texel of byte 128 at a texel centre, exactly


def occlusion_against_ao(with_ao=True):
    """a glTF quad with a constant occlusion texel (byte 128, uv on the 1 x 1 texture's centre) over an ao_in that is below, above and exactly equal to it and
    NaN in one column each; a Standard quad and uncovered pixels next to it, whose ao_out must be ao_in's bits"""
    g, t = quad(1.5, 2.5, 21.5, 20.5, uv=((0.5, 0.5),) * 4)
    st, _ = quad(24.5, 2.5, 36.5, 20.5)
    ao = np.empty((24, 40), f32)
    ao[:] = np.array([0.25, 0.75, OCC, np.nan, np.nextafter(OCC, f32(0)), np.nextafter(OCC, f32(1)), 0.0, 1.0], f32)[np.arange(40) % 8][None, :]
    s = scene(40, 24, screen_projection(40, 24), [gltf(draw(g, t, ids=[0])), draw(st, t, ids=[1])], models=[IDENTITY, IDENTITY],
              textures=[WHITE, FLAT_NORMAL, np.array([[[128, 7, 9, 255]]], np.uint8)], mats=[gltf_material(samplers=(0, 1, 0, 2, 0)), material()], inst_materials=[0, 1])
    s["ao_in"] = ao if with_ao else None
    return s


def _occlusion_reached(r, s):
    g, ao, occ = r["gltf"], r["ao_in"], r["emissive"][..., 3]
    std, unc = r["covered"] & ~g, ~r["covered"]
    same = lambda m: np.array_equal(r["ao_out"][m].view(np.uint32), ao[m].view(np.uint32))
    return (g.sum() == 20 * 18 and (occ[g] == OCC).all() and (occ[g] < ao[g]).sum() > 30 and (occ[g] > ao[g]).sum() > 30 and (occ[g] == ao[g]).sum() >= 18
            and np.isnan(ao[g]).sum() >= 18 and np.isnan(r["ao_out"][g]).sum() == np.isnan(ao[g]).sum() and std.sum() > 100 and unc.sum() > 100
            and np.isnan(ao[std]).any() and np.isnan(ao[unc]).any() and same(std) and same(unc)
            and (r["ao_out"][g & (ao > OCC)] == OCC).all() and same(g & (ao <= OCC)))


def emissive_srgb():
    """emissiveFactor x an sRGB texel; emissiveFactor[3] (123) is not read; a Standard quad and uncovered pixels keep (0, 0, 0, 1)"""
    g, t = quad(1.5, 2.5, 21.5, 20.5, uv=((0, 0), (1.5, 0), (1.5, 1.5), (0, 1.5)))
    st, _ = quad(24.5, 2.5, 36.5, 20.5)
    return scene(40, 24, screen_projection(40, 24), [gltf(draw(g, t, ids=[0])), draw(st, t, ids=[1])], models=[IDENTITY, IDENTITY],
                 textures=[WHITE, FLAT_NORMAL, rgb_texture(5, 4, 8)], srgb=[False, False, True],
                 mats=[gltf_material(emissive=(0.5, 2.0, 0.25, 123.0), samplers=(0, 1, 0, 0, 2)), material()], inst_materials=[0, 1])


def _emissive_reached(r, s):
    g = r["gltf"]
    other = dict(s, materials=s["materials"].copy())
    other["materials"].view(GLTF)["emissiveFactor"][0, 3] = -7.0
    return (g.sum() == 20 * 18 and (r["emissive"][g][:, :3].sum(axis=-1) > 0).all() and (r["emissive"][~g] == gltf_ref.NO_EMISSIVE).all() and (r["covered"] & ~g).sum() > 100
            and r["stats"]["taps"]["srgb"] > 0 and np.array_equal(gltf_ref.render(other)["emissive"], r["emissive"]))


NORMAL_SCALES = (1.0, 2.0, 0.3, -1.0, 0.0)


def normal_scales():
    """normalScale 1, 2, 0.3, -1 and 0 under a tilted normal map: 0 leaves a zero vector to normalise (NaN normals)"""
    v, t = quad(0.5, 2.5, 7.5, 20.5, uv=((0, 0), (1, 0), (1, 2), (0, 2)))
    for q in v:
        q[5:14] = (0.1, 0.2, 0.97, 0.98, 0.0, -0.1, 0.0, 0.97, -0.2)
    return scene(40, 24, screen_projection(40, 24), [gltf(draw(v, t))], models=[translation(8.0 * k, 0.0, 0.0) for k in range(5)], textures=[WHITE, tilted_normal_map(7)],
                 mats=[gltf_material(normal_scale=x) for x in NORMAL_SCALES], inst_materials=list(range(5)))


def _normal_scales_reached(r, s):
    n = r["planes"][1][..., :3]
    col = lambda k: n[3:20, 8 * k + 1: 8 * k + 7]
    return (r["covered"].sum() == 5 * 7 * 18 and np.isfinite(n[:, :32][r["covered"][:, :32]]).all() and np.isnan(col(4)).all()
            and np.abs(col(0) + col(3)).max() < 1e-6 and np.abs(col(0) - col(1)).max() < 1e-6 and np.abs(col(0)[..., 0]).max() > 0.05)


# ---- alphaCutoff ------------------------------------------------------------------------------------------------------------------------------------
T200 = f32(200) / f32(255)


def cutoff_exact():
    """1 x 1 alpha textures sampled on the texel centre under w = 1 and colour alpha 1, so alpha is the texel's value exactly: on the cutoff (kept), one ulp below
    it (discarded), alpha 0 against cutoff 0 (kept), byte 254 against cutoff 1 (discarded), a NaN cutoff (kept), a NaN alpha (kept)"""
    v, t = quad(0.5, 3.5, 5.5, 19.5, uv=((0.5, 0.5),) * 4)
    a200, a0, a254 = alpha_texture([[200]]), alpha_texture([[0]]), alpha_texture([[254]])
    mats = [gltf_material(cutoff=T200, samplers=(2, 1, 0, 0, 0)), gltf_material(cutoff=np.nextafter(T200, f32(1)), samplers=(2, 1, 0, 0, 0)),
            gltf_material(cutoff=0.0, samplers=(3, 1, 0, 0, 0)), gltf_material(cutoff=1.0, samplers=(4, 1, 0, 0, 0)),
            gltf_material(cutoff=np.nan, samplers=(3, 1, 0, 0, 0)), gltf_material(base=(1, 1, 1, np.nan), cutoff=0.5, samplers=(2, 1, 0, 0, 0))]
    return scene(40, 24, screen_projection(40, 24), [cutout(gltf(draw(v, t)))], models=[translation(6.0 * k, 0.0, 0.0) for k in range(6)],
                 textures=[WHITE, FLAT_NORMAL, a200, a0, a254], mats=mats, inst_materials=list(range(6)))


def _cutoff_exact_reached(r, s):
    kept = [r["covered"][:, 6 * k: 6 * k + 6].sum() for k in range(6)]
    return (kept == [80, 0, 80, 0, 80, 80] and r["stats"]["discarded"] == 160 and r["stats"]["on_cutoff"] == 160 and r["stats"]["nan_alpha"] == 80
            and (r["planes"][0][..., 3][:, 0:6][r["covered"][:, 0:6]] == T200).all() and (r["planes"][0][..., 3][:, 12:18][r["covered"][:, 12:18]] == 0).all())


def cutoff_per_instance():
    """one draw, three instances, three cutoffs over the same bilinear alpha ramp (0 -> 1 over 32 columns, masked_cases.bilinear_ramp_srgb's): 26, 16 and 6 columns kept"""
    v, t = quad(4.5, 0.5, 36.5, 7.5, uv=((0.25, 0.5), (0.75, 0.5), (0.75, 0.5), (0.25, 0.5)))
    return scene(40, 24, screen_projection(40, 24), [cutout(gltf(draw(v, t)))], models=[translation(0.0, 8.0 * k, 0.0) for k in range(3)],
                 textures=[alpha_texture([[0, 255]]), FLAT_NORMAL], srgb=[True, False], mats=[gltf_material(cutoff=c) for c in (0.1875, 0.5, 0.8125)],
                 inst_materials=[0, 1, 2])


def cutoff_tie_discarded():
    """masked_cases.tie_later_discarded as glTF: the later coincident triangle is discarded on half its area, the earlier order wins there"""
    s = mc.tie_later_discarded()
    s["materials"] = np.concatenate([gltf_material(), gltf_material(base=(0.5, 0.25, 0.125, 1), cutoff=0.6, samplers=(2, 1, 0, 0, 0))])
    s["draws"] = [gltf(d) for d in s["draws"]]
    return s


def cutoff_half_is_the_standard_masked_draw():
    """masked_cases.checker_over_opaque with the cutout draw as a glTF draw over the equivalent record with cutoff 0.5: Standard's keys"""
    s = mc.checker_over_opaque()
    s["materials"] = np.concatenate([s["materials"][:1], gltf_material(samplers=(2, 1, 0, 0, 0), cutoff=0.5)])
    s["draws"] = [s["draws"][0], gltf(s["draws"][1])]
    return s


def large_cutout_two_superblocks():
    """masked_cases.large_checker_two_superblocks as glTF with cutoff 0.3: the wave path of the draw kernel with the threshold carried along"""
    s = mc.large_checker_two_superblocks()
    s["materials"] = gltf_material(cutoff=0.3, emissive=(1, 1, 1, 1), samplers=(0, 1, 0, 0, 0))
    s["draws"] = [gltf(d) for d in s["draws"]]
    return s


# ---- both shaders in one pass -----------------------------------------------------------------------------------------------------------------------
def mixed_pass():
    """Standard, Standard cutout, glTF and glTF cutout draws in one pass over one table that holds both records; the same triangle drawn by a Standard and then
    by a glTF draw (a depth tie the glTF one wins) and, elsewhere, by a glTF and then a Standard draw (the Standard one wins)"""
    tri = [vertex((2.2, 1.3, 0.4), (0.0, 0.0)), vertex((17.7, 3.3, 0.6), (1.0, 0.0)), vertex((9.9, 12.2, 0.7), (0.5, 1.0))]
    q, t = quad(21.3, 12.2, 38.6, 22.7, z=0.5, uv=((0, 0), (2, 0), (2, 2), (0, 2)))
    models = [IDENTITY, IDENTITY, translation(20.0, 0.0, 0.0), translation(20.0, 0.0, 0.0), IDENTITY, translation(-20.0, 0.0, 0.0)]
    mats = [material(albedo=(0.9, 0.5, 0.3, 1)), gltf_material(base=(0.2, 0.4, 0.8, 1), emissive=(1, 0.5, 0.25, 0), samplers=(0, 1, 2, 2, 2)),
            material(samplers=(3, 0, 1, 0)), gltf_material(cutoff=0.3, emissive=(0.1, 0.2, 0.3, 0), samplers=(3, 1, 2, 2, 2))]
    draws = [draw(tri, [(0, 1, 2)], ids=[0]), gltf(draw(tri, [(0, 1, 2)], ids=[1])),          # the tie, glTF later
             gltf(draw(tri, [(0, 1, 2)], ids=[2])), draw(tri, [(0, 1, 2)], ids=[3]),          # the tie, Standard later
             cutout(draw(q, t, ids=[4])), cutout(gltf(draw(q, t, ids=[5])))]
    s = scene(40, 24, screen_projection(40, 24), draws, models=models, textures=[WHITE, FLAT_NORMAL, rgb_texture(3, 3, 4), checker()], srgb=[False, False, True, False],
              mats=mats, inst_materials=[0, 1, 1, 0, 2, 3])
    s["ao_in"] = np.random.default_rng(2).uniform(0, 1, (24, 40)).astype(f32)
    return s


def _mixed_reached(r, s):
    own = (r["keys"] & LOW).astype(np.int64)
    left, right = own[:12, :20], own[:12, 20:]
    return (set(np.unique(left)) == {0, 3} and set(np.unique(right)) == {0, 7} and r["gltf"][:12, :20][left == 3].all() and not r["gltf"][:12, 20:][right == 7].any()
            and r["stats"]["ties"] > 100 and r["stats"]["discarded"] > 50 and (r["cutout"] & r["gltf"]).sum() > 20 and (r["cutout"] & ~r["gltf"]).sum() > 20
            and (r["emissive"][..., :3][r["gltf"]].sum(axis=-1) > 0).all())


def table_edges():
    """a materialInstance beyond the table (slot 0, read as the glTF record), each of the five sampler indices beyond the table (descriptor 0), and a descriptor
    without texels behind each of occlusion and emissive (samples 0)"""
    v, t = quad(0.5, 2.5, 4.5, 20.5, uv=((0, 0), (1, 0), (1, 1), (0, 1)))
    base = dict(base=(0.9, 0.8, 0.7, 1), emissive=(1, 1, 1, 0), metallic=0.5, roughness=0.25)
    far = [(9, 1, 2, 2, 2), (2, 77, 2, 2, 2), (2, 1, 4, 2, 2), (2, 1, 2, 0xFFFFFFFF, 2), (2, 1, 2, 2, 5)]
    mats = [gltf_material(samplers=(2, 1, 2, 2, 2), **base)] + [gltf_material(samplers=x, **base) for x in far] + [gltf_material(samplers=(2, 1, 2, 3, 3), **base)]
    return scene(40, 24, screen_projection(40, 24), [gltf(draw(v, t))], models=[translation(5.0 * k, 0.0, 0.0) for k in range(8)],
                 textures=[rgb_texture(2, 2, 1), FLAT_NORMAL, rgb_texture(3, 2, 5), NO_TEXELS], srgb=[True, False, False, False], mats=mats,
                 inst_materials=[0, 1, 2, 3, 4, 5, 6, 40])


def _table_edges_reached(r, s):
    p = r["planes"]
    col = lambda a, k: a[3:20, 5 * k + 1: 5 * k + 4]
    differs = lambda a, k: not np.array_equal(col(a, k), col(a, 0))
    return (r["covered"].sum() == 8 * 4 * 18 and r["stats"]["beyond_table"] >= 5 and r["stats"]["materials"] == {0, 1, 2, 3, 4, 5, 6, 40}
            and differs(p[2][..., :3], 1) and differs(p[1][..., :3], 2) and differs(p[2][..., 3], 3) and differs(r["emissive"][..., 3], 4)
            and differs(r["emissive"][..., :3], 5) and (col(r["emissive"], 6) == 0).all() and (col(r["ao_out"], 6) == 0).all()
            and np.array_equal(col(p[2], 7), col(p[2], 0)) and np.array_equal(col(r["emissive"], 7), col(r["emissive"], 0)))


# ---- random -----------------------------------------------------------------------------------------------------------------------------------------
NUM_SOUPS = 12


def gltf_soup(seed):
    """masked_cases.masked_soup with a table that holds both records at random, each draw flagged glTF and / or cutout at random (at least one glTF draw), random
    cutoffs, normal scales and emissive factors, and a random ao_in with a few NaN.  An instance may point a draw at a slot built as the other record: the
    flag decides how it is read."""
    s = mc.masked_soup(seed)
    rng = np.random.default_rng(9000 + seed)
    slots = []
    for m in s["materials"]:
        if rng.integers(0, 3) == 0:
            slots.append(m.reshape(1))
        else:
            slots.append(gltf_material(base=(*rng.uniform(0, 1, 3), rng.uniform(0.8, 1.6)), emissive=rng.uniform(0, 2, 4), metallic=rng.uniform(), roughness=rng.uniform(),
                                       normal_scale=rng.choice([1.0, 0.5, -1.0, 2.0]), cutoff=rng.choice([0.0, 0.3, 0.5, 0.9]), samplers=rng.integers(0, 5, 5)))
    s["materials"] = np.concatenate(slots)
    flags = [(bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for _ in s["draws"]]
    flags[int(rng.integers(0, len(flags)))] = (True, bool(seed & 1))
    s["draws"] = [cutout(gltf(d, g), c) for d, (g, c) in zip(s["draws"], flags)]
    ao = rng.uniform(0, 1, (s["H"], s["W"])).astype(f32)
    ao[rng.integers(0, s["H"], 5), rng.integers(0, s["W"], 5)] = np.nan
    s["ao_in"] = ao
    return s


CASES = {
    "normal_matrix_models": (normal_matrix_models, _normal_matrix_reached),
    "normal_matrix_near_plane": (normal_matrix_near_plane, lambda r, s: r["stats"]["cut_one"] >= 1 and r["stats"]["cut_two"] >= 2 and r["gltf"].sum() > 100
                                 and any(x and x % 2 == 0 for x in orders(r))
                                 and (np.abs(r["planes"][1][..., :3] - gltf_ref.render(s, standard_basis=True)["planes"][1][..., :3]).max(axis=-1)[r["gltf"]] > 1e-2).mean() > 0.9),
    "orm_channels": (orm_channels, _orm_reached),
    "occlusion_against_ao": (occlusion_against_ao, _occlusion_reached),
    "occlusion_without_ao_in": (lambda: occlusion_against_ao(False), lambda r, s: s["ao_in"] is None and (r["ao_in"] == 1).all() and (r["ao_out"][r["gltf"]] == OCC).all()
                                and (r["ao_out"][~r["gltf"]] == 1).all() and r["gltf"].sum() == 360),
    "emissive_srgb": (emissive_srgb, _emissive_reached),
    "normal_scales": (normal_scales, _normal_scales_reached),
    "cutoff_exact": (cutoff_exact, _cutoff_exact_reached),
    "cutoff_per_instance": (cutoff_per_instance, lambda r, s: [int(r["covered"][8 * k: 8 * k + 8].sum()) for k in range(3)] == [26 * 7, 16 * 7, 6 * 7]
                            and r["stats"]["on_cutoff"] == 21 and r["stats"]["taps"]["srgb"] > 0),
    "cutoff_tie_discarded": (cutoff_tie_discarded, lambda r, s: r["stats"]["discarded_at_tie"] > 50 and orders(r) == {0, 1, 3}),
    "cutoff_half_is_the_standard_masked_draw": (cutoff_half_is_the_standard_masked_draw,
                                                lambda r, s: r["stats"]["discarded"] > 100 and (r["cutout"] & r["gltf"]).sum() > 100
                                                and np.array_equal(r["keys"], masked_ref.render(mc.checker_over_opaque())["keys"])),
    "large_cutout_two_superblocks": (large_cutout_two_superblocks, lambda r, s: r["stats"]["large"] >= 1 and r["stats"]["discarded"] > 500 and r["covered"].sum() > 1000
                                     and r["covered"][:, :64].any() and r["covered"][:, 64:].any() and r["covered"][64:].any()
                                     and not np.array_equal(r["covered"], masked_ref.render(mc.large_checker_two_superblocks())["covered"])),
    "mixed_pass": (mixed_pass, _mixed_reached),
    "table_edges": (table_edges, _table_edges_reached),
}
CULL_BACK_CASES = ("normal_matrix_models", "normal_matrix_near_plane", "cutoff_tie_discarded", "mixed_pass")   # (the first two keep their front faces, the last two lose everything)
BAND_CASES = ("normal_matrix_models", "normal_matrix_near_plane", "large_cutout_two_superblocks")   # 72 x 40 and 96 x 72: more than one tile row
GOLDEN_CASES = ("mixed_pass", "normal_matrix_models", "cutoff_exact")


def all_scenes():
    """name -> scene, the cases and the soups"""
    out = {name: build() for name, (build, _) in CASES.items()}
    out.update({f"gltf_soup_{seed}": gltf_soup(seed) for seed in range(NUM_SOUPS)})
    return out


def opaque_prepass(s):
    """the Opaque depth prepass: the project's oracle over the draws without ALPHA_CUTOUT (the position transform is the same in both shaders)"""
    return mc.opaque_prepass(s)


def full_prepass(s):
    """DepthPrepass Opaque, then Masked (each cutout draw against its own shader's threshold): what a RenderScene pass of the scene starts from"""
    cut = dict(s, draws=[d for d in s["draws"] if d.get("alpha_cutout", False)])
    return gltf_ref.render(cut, prepass=opaque_prepass(s))["depth"]


# ---- a scene as flat arrays (the golden file's inputs) and back ---------------------------------------------------------------------------------------
def scene_to_arrays(s, prefix):
    out = sc.scene_to_arrays(s, prefix)
    out[f"{prefix}.flags"] = np.array([[d.get("alpha_cutout", False), d.get("gltf", False)] for d in s["draws"]], np.uint8).reshape(-1, 2)
    if s.get("ao_in") is not None:
        out[f"{prefix}.ao_in"] = s["ao_in"]
    return out


def scene_from_arrays(g, prefix):
    s = sc.scene_from_arrays(g, prefix)
    for d, (c, gl) in zip(s["draws"], g[f"{prefix}.flags"]):
        d["alpha_cutout"], d["gltf"] = bool(c), bool(gl)
    s["ao_in"] = g[f"{prefix}.ao_in"] if f"{prefix}.ao_in" in g else None
    return s
