"""The scenes of the surface-pass tests (tests/test_surface_cpu.py, tests/test_surface_gpu.py), at the smallest sizes at which the kernels can still go
wrong: frames of 40 x 24, 37 x 21 and 72 x 40 (odd, no multiples of 8, 16 or 64) and one of 200 x 136 for a triangle larger than the frame.  A scene is the
dict tests/surface_ref.py describes; CASES maps a name to (builder, what the case must reach: a predicate over the restatement's stats and result).

Two kinds of camera: `screen` scenes are looked at through an orthographic matrix in pixel units (clip w = 1; a vertex (x, y) lands on the 1/256 grid at
exactly x, y), which puts vertices and edges exactly on pixel centres; `camera` scenes use the reversed-Z perspective projection of
sailor_amd.synth.perspective_reversed_z with the eye at the origin looking down -z."""
import numpy as np

from sailor_amd import _lib, host, synth

f32 = np.float32
IDENTITY = np.eye(4, dtype=f32).reshape(16)
FLAT_NORMAL = np.array([[[128, 128, 255, 255]]], np.uint8)
WHITE = np.array([[[255, 255, 255, 255]]], np.uint8)


# ---- building blocks ------------------------------------------------------------------------------------------------------------------------------
def vertex(pos, uv=(0, 0), color=(1, 1, 1, 1), normal=(0, 0, 1), tangent=(1, 0, 0), bitangent=(0, 1, 0)):
    return np.array([*uv, *pos, *normal, *tangent, *bitangent, *color], f32)


def screen_projection(W, H):
    """pixel (x, y) with depth z -> clip (2x / W - 1, 1 - 2y / H, z, 1): window x, y = the input on the 1/256 grid"""
    m = np.zeros(16, f32)
    m[0], m[5], m[10], m[15], m[12], m[13] = 2.0 / W, -2.0 / H, 1.0, 1.0, -1.0, 1.0
    return m


def translation(x, y, z):
    m = np.eye(4, dtype=f32)
    m[3, 0:3] = (x, y, z)      # column-major: row 3 of the array = column 3 of the matrix
    return m.reshape(16)


def instances(models, materials=None):
    a = np.zeros(len(models), host.INSTANCE_DTYPE)
    a["model"] = np.asarray(models, f32).reshape(-1, 16)
    a["materialInstance"] = 0 if materials is None else materials
    return a


def material(albedo=(1, 1, 1, 1), metallic=1.0, roughness=1.0, samplers=(0, 0, 1, 0)):
    """samplers = (albedo, metalness, normal, roughness)"""
    m = np.zeros(1, np.dtype(_lib.MATERIAL_DTYPE))
    m["albedo"], m["metallic"], m["roughness"] = albedo, metallic, roughness
    m["albedoSampler"], m["metalnessSampler"], m["normalSampler"], m["roughnessSampler"] = samplers
    return m


def draw(vertices, indices, ids=None, first_instance=0, num_drawn=None, cull_back=False):
    return dict(vertices=np.asarray(vertices, f32).reshape(-1, 18), indices=np.asarray(indices, np.uint32).reshape(-1, 3),
                instance_ids=None if ids is None else np.asarray(ids, np.uint32), first_instance=first_instance, num_drawn=num_drawn, cull_back=cull_back)


def scene(W, H, projection, draws, models=(IDENTITY,), view=IDENTITY, mats=None, textures=None, srgb=None, inst_materials=None, prim_base=0):
    textures = [WHITE, FLAT_NORMAL] if textures is None else textures
    return dict(W=W, H=H, view=np.asarray(view, f32), projection=np.asarray(projection, f32), instances=instances(models, inst_materials),
                materials=np.concatenate(mats) if mats is not None else material(), textures=textures,
                srgb=[False] * len(textures) if srgb is None else srgb, draws=draws, prim_base=prim_base)


def distinct_texture(w, h, seed):
    """every texel different from every other in every channel pattern"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    t[..., 0] = (np.arange(w * h).reshape(h, w) * 255 // max(w * h - 1, 1)).astype(np.uint8)
    return t


def quad(x0, y0, x1, y1, z=0.5, uv=((0, 0), (1, 0), (1, 1), (0, 1)), colors=None, zs=None):
    """the rectangle as vertices 0..3 (x0y0, x1y0, x1y1, x0y1) and two triangles (0, 1, 2), (0, 2, 3)"""
    zs = [z] * 4 if zs is None else zs
    colors = [(1, 1, 1, 1)] * 4 if colors is None else colors
    p = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return [vertex((p[k][0], p[k][1], zs[k]), uv[k], colors[k]) for k in range(4)], [(0, 1, 2), (0, 2, 3)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def shared_edge_quad():
    """two triangles of a quad whose corners and diagonal run through pixel centres: every pixel of it exactly once"""
    v, t = quad(3.5, 2.5, 30.5, 20.5)
    return scene(40, 24, screen_projection(40, 24), [draw(v, t)])


def fan_around_a_pixel_centre():
    """six triangles around a vertex that sits exactly on a pixel centre, the rim on pixel centres too"""
    c = (18.5, 10.5)
    rim = [(30.5, 10.5), (24.5, 19.5), (10.5, 18.5), (4.5, 10.5), (11.5, 1.5), (25.5, 2.5)]
    v = [vertex((*c, 0.5))] + [vertex((*p, 0.5)) for p in rim]
    return scene(37, 21, screen_projection(37, 21), [draw(v, [(0, 1 + k, 1 + (k + 1) % 6) for k in range(6)])])


def _tie_vertices():
    return [vertex((4.2, 3.1, 0.4), color=(1, 0, 0, 1)), vertex((33.7, 5.3, 0.6), color=(0, 1, 0, 1)), vertex((17.9, 21.2, 0.7), color=(0, 0, 1, 1))]


def tie_twice_in_one_draw():
    """the same triangle twice in one draw: the later one owns every pixel"""
    return scene(40, 24, screen_projection(40, 24), [draw(_tie_vertices(), [(0, 1, 2), (0, 1, 2)])])


def tie_two_instances():
    """... in two instances with different materials"""
    return scene(40, 24, screen_projection(40, 24), [draw(_tie_vertices(), [(0, 1, 2)])], models=(IDENTITY, IDENTITY),
                 mats=[material(), material(albedo=(0.5, 0.25, 0.125, 1))], inst_materials=[0, 1])


def tie_two_draws():
    return scene(40, 24, screen_projection(40, 24), [draw(_tie_vertices(), [(0, 1, 2)]), draw(_tie_vertices(), [(0, 1, 2)])])


def tie_coplanar_reversed_indices():
    """a coplanar pair, the second listed in reversed index order (other winding, other vertex roles): the later one still wins"""
    v = _tie_vertices()
    for q in v:
        q[4] = 0.5   # one depth everywhere: interpolated in another vertex order a sloped plane rounds differently, and the later one would lose some pixels
    return scene(40, 24, screen_projection(40, 24), [draw(v, [(0, 1, 2), (2, 1, 0)])])


def nearer_drawn_first():
    """a nearer (larger z) triangle drawn first keeps its pixels"""
    near, far = quad(8.3, 4.2, 30.1, 19.7, z=0.8), quad(2.3, 1.2, 36.1, 22.7, z=0.3)
    return scene(40, 24, screen_projection(40, 24), [draw(near[0] + far[0], near[1] + [(4, 5, 6), (4, 6, 7)])])


def instance_indirection():
    """instance ids permuted and repeated, and a second draw with firstInstance > 0; every instance its own material"""
    v, t = quad(0.0, 0.0, 9.3, 7.1, z=0.5)
    models = [translation(4.0 * k, 2.5 * k, 0.01 * k) for k in range(6)]
    return scene(40, 24, screen_projection(40, 24), [draw(v, t, ids=[4, 1, 1, 3, 0, 4]), draw(v, t, first_instance=2, num_drawn=3)], models=models,
                 mats=[material(albedo=(k / 6 + 0.1, 1 - k / 6, 0.5, 1)) for k in range(6)], inst_materials=list(range(6)))


def camera_projection(W, H, near=1.0):
    return synth.perspective_reversed_z(W, H, near)


def near_plane():
    """triangles with one vertex beyond the near plane, with two, and with one behind the eye; every vertex its own colour and texcoord"""
    col = [(1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 1, 1)]
    uvs = [(0, 0), (1, 0), (0, 1)]
    tris = [[(-1.5, -0.5, -3.0), (-0.2, -0.7, -0.4), (-0.9, 0.8, -2.5)],     # one beyond
            [(0.3, -0.6, -0.5), (1.6, -0.4, -0.6), (1.0, 0.9, -3.5)],        # two beyond
            [(-0.4, 0.2, -2.0), (0.5, 0.3, -2.2), (0.1, 0.4, 1.5)]]          # one behind the eye
    v = [vertex(p, uvs[k], col[k]) for tri in tris for k, p in enumerate(tri)]
    return scene(72, 40, camera_projection(72, 40), [draw(v, [(0, 1, 2), (3, 5, 4), (6, 7, 8)])])   # (the second one wound the other way)


def oblique_quad():
    """a quad tilted against the view under a scaling, rotating, moving model, whose texcoord equals its world x, y (computed in float64, rounded once):
    uv == worldPos.xy must survive the interpolation"""
    p = [(-2.0, -1.5, -2.0), (3.0, -1.0, -6.0), (2.5, 2.0, -9.0), (-1.5, 1.0, -3.0)]
    model = host.transform_matrix([0.3, -0.2, -0.5, 1.0], [0.0, 0.0, 0.0872, 0.9962], [1.3, 0.7, 1.1, 1.0])
    M = np.asarray(model, np.float64).reshape(4, 4).T
    world = [M @ np.array([*np.asarray(q, f32).astype(np.float64), 1.0]) for q in p]
    v = [vertex(q, (w[0], w[1])) for q, w in zip(p, world)]
    return scene(72, 40, camera_projection(72, 40), [draw(v, [(0, 1, 2), (0, 2, 3)])], models=[model])


def grazing_quad():
    """a ground quad seen at a grazing angle: clip w from 1 to 50 across it"""
    p = [(-1.0, -0.5, -1.0), (1.0, -0.5, -1.0), (40.0, -0.4, -50.0), (-40.0, -0.4, -50.0)]
    v = [vertex(q, (q[0] * 0.25, q[2] * 0.25), c) for q, c in zip(p, [(1, 0, 0, 1), (0, 1, 0, 1), (0, 0, 1, 1), (1, 1, 0, 0.5)])]
    return scene(72, 40, camera_projection(72, 40), [draw(v, [(0, 1, 2), (0, 2, 3)])], textures=[distinct_texture(16, 16, 3), FLAT_NORMAL])


def degenerates():
    """zero-area triangles, all vertices off screen, w <= 0 everywhere, a NaN position -- and one ordinary triangle so that the frame is not empty"""
    tris = [[(-1, -1, -4), (0, 0, -4), (1, 1, -4)], [(0.5, 0.5, -3), (0.5, 0.5, -3), (0.2, 0.1, -3)],          # zero area
            [(50, 40, -2), (60, 40, -2), (55, 50, -2)], [(-1, -1, 2), (1, -1, 3), (0, 1, 2.5)],                     # off screen; behind the eye
            [(np.nan, 0, -2), (1, 0, -2), (0, 1, -2)], [(0, 0, 0), (1, 0, 0), (0, 1, 0)],                           # NaN; w == 0
            [(-0.8, -0.6, -2), (0.9, -0.5, -2), (0.1, 0.7, -2)]]
    v = [vertex(p) for tri in tris for p in tri]
    return scene(72, 40, camera_projection(72, 40), [draw(v, np.arange(len(v)).reshape(-1, 3))])


def _texture_scene(uv_rect, albedo_sampler, textures, srgb, W=40, H=24):
    (u0, v0), (u1, v1) = uv_rect
    v, t = quad(0.0, 0.0, float(W), float(H), uv=((u0, v0), (u1, v0), (u1, v1), (u0, v1)))
    n = len(textures)
    return scene(W, H, screen_projection(W, H), [draw(v, t)], textures=textures, srgb=srgb,
                 mats=[material(albedo=(0.9, 0.8, 0.7, 0.6), metallic=0.5, roughness=0.75, samplers=(albedo_sampler, 1 % n, 2 % n, albedo_sampler))])


TEXTURE_SET = [distinct_texture(16, 16, 1), distinct_texture(2, 3, 2), np.array([[[200, 100, 50, 25]]], np.uint8), FLAT_NORMAL]


def texture_on_texel_centres_and_edges():
    """uv exactly on texel centres and on texel edges, both at 0 and at 1, in u and in v: the quad's corners sit on pixel centres 64 x 32 pixels apart and uv
    runs from 0 to 2 over them, so pixel (i, j) has uv = (i / 32, j / 16) exactly (powers of two: nothing rounds); over the 16 x 8 texture u * 16 - 0.5 =
    i / 2 - 0.5 -- even i on a texel edge (tap weight 0.5; i = 0 is u = 0, i = 32 is u = 1, both with the second tap wrapped round), odd i on a texel
    centre (weight 0) -- and the same in v"""
    v, t = quad(0.5, 0.5, 64.5, 32.5, uv=((0, 0), (2, 0), (2, 2), (0, 2)))
    tex = [distinct_texture(16, 8, 6), FLAT_NORMAL]
    return scene(72, 40, screen_projection(72, 40), [draw(v, t)], textures=tex, srgb=[True, False],
                 mats=[material(albedo=(0.9, 0.8, 0.7, 0.6), metallic=0.5, roughness=0.75, samplers=(0, 0, 1, 0))])


def texture_below_0_above_1():
    return _texture_scene(((-1.25, -0.5), (2.5, 1.75)), 0, TEXTURE_SET, [False] * 4)


def texture_2x3_srgb():
    return _texture_scene(((-0.5, -0.5), (1.5, 1.5)), 1, TEXTURE_SET, [True, True, False, False])


def texture_1x1():
    return _texture_scene(((0, 0), (1, 1)), 2, TEXTURE_SET, [False, False, True, False])


def texture_last_and_beyond():
    """albedo from the last descriptor, metalness / roughness from an index beyond the table (reads descriptor 0)"""
    s = _texture_scene(((0, 0), (3, 2)), 3, TEXTURE_SET, [True, False, False, False])
    s["materials"]["metalnessSampler"], s["materials"]["roughnessSampler"] = 4, 0xFFFFFFFF
    return s


def texture_nan_uv():
    s = _texture_scene(((0, 0), (1, 1)), 0, TEXTURE_SET, [False] * 4)
    s["draws"][0]["vertices"][1, 0] = np.nan   # (vertex 1 belongs to the first triangle only)
    return s


def materials_and_normal_map():
    """materialInstance per instance, a normal map that tilts the normal, a tangent basis from a non-uniformly scaled, rotated model"""
    rng = np.random.default_rng(5)
    nm = rng.integers(60, 200, (4, 4, 4), dtype=np.uint8)
    nm[..., 2] = 230
    p = [(-1.0, -1.0, 0.0), (1.0, -1.0, 0.0), (1.0, 1.0, 0.0), (-1.0, 1.0, 0.0)]
    v = [vertex(q, (0.5 * q[0] + 0.5, 0.5 * q[1] + 0.5), normal=(0.1, 0.2, 0.97), tangent=(0.98, 0.0, -0.1), bitangent=(0.0, 0.97, -0.2)) for q in p]
    models = [host.transform_matrix([-1.2, 0.2, -4.0, 1.0], [0.18, 0.37, 0.09, 0.907], [1.5, 0.6, 1.0, 1.0]),
              host.transform_matrix([1.3, -0.3, -5.0, 1.0], [-0.3, 0.1, 0.2, 0.927], [0.7, 1.9, 1.0, 1.0])]
    return scene(72, 40, camera_projection(72, 40), [draw(v, [(0, 1, 2), (0, 2, 3)])], models=models, textures=[distinct_texture(16, 16, 9), nm, WHITE],
                 srgb=[True, False, False], mats=[material(samplers=(0, 2, 1, 2)), material(albedo=(0.3, 0.6, 0.9, 0.8), metallic=0.2, roughness=0.4, samplers=(2, 0, 1, 0))],
                 inst_materials=[0, 1])


def _two_meshes(prim_base):
    qa, ta = quad(2.2, 1.3, 20.6, 15.2, z=0.4)
    tri = [vertex((10.1, 20.3, 0.6), color=(1, 0, 0, 1)), vertex((35.2, 22.1, 0.5), color=(0, 1, 0, 1)), vertex((28.3, 3.2, 0.7), color=(0, 0, 1, 1))]
    models = [IDENTITY, translation(6.0, 3.0, 0.1), translation(-3.0, 2.0, 0.2)]
    return scene(40, 24, screen_projection(40, 24), [draw(qa, ta, ids=[0, 1]), draw(tri, [(0, 1, 2)], ids=[2, 0]), draw(qa, ta, ids=[2])], models=models,
                 mats=[material(), material(albedo=(0.2, 0.4, 0.8, 1)), material(albedo=(0.9, 0.1, 0.3, 1))], inst_materials=[0, 1, 2], prim_base=prim_base)


def multiple_draws():
    """two meshes, three draws: primBase chains from draw to draw"""
    return _two_meshes(0)


def multiple_draws_high_prim_base():
    """... with primBase close under 2^32: the high end of the key's low word (the three draws add 8 + 4 + 4 primitives: the last order is 2^32 - 3)"""
    return _two_meshes(2 ** 32 - 2 - 16)


def triangle_larger_than_the_frame():
    """one triangle that covers the whole 200 x 136 frame (handed round the wave over several 64-texel spans) and a small one in front"""
    big = [vertex((-300.0, -200.0, 0.2), (0, 0), (1, 0, 0, 1)), vertex((700.0, -150.0, 0.4), (4, 0), (0, 1, 0, 1)), vertex((100.0, 600.0, 0.3), (0, 4), (0, 0, 1, 1))]
    small = [vertex((90.3, 60.2, 0.9)), vertex((120.1, 64.7, 0.9)), vertex((101.4, 90.9, 0.9))]
    return scene(200, 136, screen_projection(200, 136), [draw(big + small, [(0, 1, 2), (3, 4, 5)])], textures=[distinct_texture(16, 16, 4), FLAT_NORMAL])


def empty_frame():
    return scene(37, 21, screen_projection(37, 21), [draw([vertex((0, 0, 0.5))] * 3, np.zeros((0, 3), np.uint32))])


def constant_material_quad():
    """a full-screen quad through the camera, one material, 1 x 1 textures: the closed-form case"""
    z = -3.0
    p = [(-12.0, -9.0, z), (12.0, -9.0, z), (12.0, 9.0, z), (-12.0, 9.0, z)]
    v = [vertex(q, (0.3, 0.6), (0.8, 0.7, 0.6, 0.9), normal=(0, 0, 1), tangent=(1, 0, 0), bitangent=(0, 1, 0)) for q in p]
    tex = [np.array([[[200, 150, 100, 250]]], np.uint8), np.array([[[150, 110, 240, 255]]], np.uint8)]
    return scene(40, 24, camera_projection(40, 24), [draw(v, [(0, 1, 2), (0, 2, 3)])], textures=tex, srgb=[True, False],
                 mats=[material(albedo=(0.9, 0.5, 0.25, 0.75), metallic=0.6, roughness=0.35, samplers=(0, 0, 1, 0))],
                 models=[host.transform_matrix([0.1, -0.2, 0.0, 1.0], [0.0, 0.0, 0.2588, 0.9659], [1.0, 1.0, 1.0, 1.0])])


def random_soup(seed):
    """a soup of <= 64 triangles around the eye (sizes over decades, some across the near plane), <= 8 instances, 2 draws, random materials and textures"""
    rng = np.random.default_rng(1000 + seed)
    W, H = [(40, 24), (37, 21), (72, 40)][seed % 3]
    nt = int(rng.integers(8, 65))
    centre = np.stack([rng.uniform(-2, 2, nt), rng.uniform(-1.5, 1.5, nt), rng.uniform(-8, 0.5, nt)], 1)[:, None, :]
    pos = (centre + rng.uniform(-1, 1, (nt, 3, 3)) * (10.0 ** rng.uniform(-1.5, 0.7, nt))[:, None, None]).reshape(-1, 3)
    v = np.zeros((3 * nt, 18), f32)
    v[:, 0:2] = rng.uniform(-2, 3, (3 * nt, 2)); v[:, 2:5] = pos; v[:, 5:14] = rng.uniform(-1, 1, (3 * nt, 9)); v[:, 14:18] = rng.uniform(0, 1, (3 * nt, 4))
    ni = int(rng.integers(1, 9))
    models = [host.transform_matrix([*rng.uniform(-1, 1, 2), rng.uniform(-3, 0), 1.0], (lambda q: q / np.linalg.norm(q))(rng.normal(size=4)),
                                    [*rng.uniform(0.5, 1.5, 3), 1.0]) for _ in range(ni)]
    tex = [distinct_texture(int(rng.integers(1, 9)), int(rng.integers(1, 9)), seed * 7 + k) for k in range(4)]
    mats = [material(albedo=rng.uniform(0, 1, 4), metallic=rng.uniform(), roughness=rng.uniform(), samplers=rng.integers(0, 5, 4)) for _ in range(3)]
    idx = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    half = nt // 2
    return scene(W, H, camera_projection(W, H, 0.5), [draw(v, idx[:half], ids=rng.integers(0, ni, int(rng.integers(1, 5)))),
                                                      draw(v, idx[half:], ids=rng.integers(0, ni, int(rng.integers(1, 5))), cull_back=bool(seed & 1))],
                 models=models, textures=tex, srgb=[bool(b) for b in rng.integers(0, 2, 4)], mats=mats, inst_materials=rng.integers(0, 4, ni))


def boxes_and_ground(num_boxes, W, H, seed=11):
    """the timing scene: num_boxes boxes over a ground quad, one draw each (the tests' box scene: synth.unit_cube_mesh under random transforms)"""
    rng = np.random.default_rng(seed)
    p, tris = synth.unit_cube_mesh()
    v = np.zeros((8, 18), f32)
    v[:, 2:5] = p; v[:, 0:2] = p[:, 0:2] * 0.5 + 0.5; v[:, 5:8] = p / np.sqrt(3); v[:, 8:11] = (1, 0, 0); v[:, 11:14] = (0, 1, 0); v[:, 14:18] = 1
    models = [host.transform_matrix([rng.uniform(-60, 60), rng.uniform(-1, 6), rng.uniform(-120, -6), 1.0], (lambda q: q / np.linalg.norm(q))(rng.normal(size=4)),
                                    [*rng.uniform(0.3, 1.5, 3), 1.0]) for _ in range(num_boxes)] + [IDENTITY]
    g = [vertex((-200, -2, -1), (0, 0)), vertex((200, -2, -1), (50, 0)), vertex((200, -2, -300), (50, 50)), vertex((-200, -2, -300), (0, 50))]
    return scene(W, H, camera_projection(W, H, 0.5), [draw(v, tris, first_instance=0, num_drawn=num_boxes, cull_back=True),
                                                      draw(g, [(0, 1, 2), (0, 2, 3)], first_instance=num_boxes, num_drawn=1)],
                 models=models, textures=[distinct_texture(16, 16, 2), FLAT_NORMAL, distinct_texture(8, 8, 3)], srgb=[True, False, True],
                 mats=[material(samplers=(0, 2, 1, 2)), material(albedo=(0.5, 0.7, 0.4, 1), samplers=(2, 0, 1, 0))],
                 inst_materials=[k % 2 for k in range(num_boxes)] + [1])


# name -> (builder, cull_back variants, what the restatement's result must show: the case reaches what it was built to reach)
CASES = {
    "shared_edge_quad": (shared_edge_quad, lambda r: r["stats"]["overwritten"] == 0 and r["covered"].sum() == 27 * 18),
    "fan_around_a_pixel_centre": (fan_around_a_pixel_centre, lambda r: r["stats"]["overwritten"] == 0 and r["covered"][10, 18]),
    "tie_twice_in_one_draw": (tie_twice_in_one_draw, lambda r: r["stats"]["ties"] > 0 and set(np.unique(r["keys"] & np.uint64(0xFFFFFFFF))) == {0, 3}),
    "tie_two_instances": (tie_two_instances, lambda r: r["stats"]["ties"] > 0 and set(np.unique(r["keys"] & np.uint64(0xFFFFFFFF))) == {0, 3}),
    "tie_two_draws": (tie_two_draws, lambda r: r["stats"]["ties"] > 0 and set(np.unique(r["keys"] & np.uint64(0xFFFFFFFF))) == {0, 3}),
    "tie_coplanar_reversed_indices": (tie_coplanar_reversed_indices, lambda r: r["stats"]["ties"] > 0 and set(np.unique(r["keys"] & np.uint64(0xFFFFFFFF))) == {0, 3}),
    "nearer_drawn_first": (nearer_drawn_first, lambda r: {1, 3, 5, 7} <= set(np.unique(r["keys"] & np.uint64(0xFFFFFFFF)))),
    "instance_indirection": (instance_indirection, lambda r: r["stats"]["ties"] > 0 and len(r["stats"]["materials"]) == 5),
    "near_plane": (near_plane, lambda r: r["stats"]["cut_one"] >= 1 and r["stats"]["cut_two"] >= 2 and 2 in set(np.unique(r["keys"] & np.uint64(1)) + 1)),
    "oblique_quad": (oblique_quad, lambda r: r["covered"].sum() > 150),
    "grazing_quad": (grazing_quad, lambda r: r["covered"].sum() > 300),
    "degenerates": (degenerates, lambda r: r["stats"]["degenerate"] >= 4 and r["stats"]["clipped_away"] >= 1 and r["covered"].any()),
    "texture_on_texel_centres_and_edges": (texture_on_texel_centres_and_edges,
                                           lambda r: r["covered"].sum() == 64 * 32 and all(r["stats"]["taps"][k] > 0 for k in
                                                                                            ("u0", "u1", "v0", "v1", "ax0", "ax_half", "ay0", "ay_half", "wrap_x", "wrap_y"))),
    "texture_below_0_above_1": (texture_below_0_above_1, lambda r: r["covered"].all() and r["stats"]["taps"]["below"] > 0 and r["stats"]["taps"]["above"] > 0
                                and r["stats"]["taps"]["wrap_x"] > 0 and r["stats"]["taps"]["wrap_y"] > 0),
    "texture_2x3_srgb": (texture_2x3_srgb, lambda r: r["covered"].all() and r["stats"]["taps"]["srgb"] > 0 and r["stats"]["taps"]["below"] > 0 and r["stats"]["taps"]["above"] > 0),
    "texture_1x1": (texture_1x1, lambda r: r["covered"].all() and r["stats"]["taps"]["wrap_x"] > 0 and r["stats"]["taps"]["wrap_y"] > 0),
    "texture_last_and_beyond": (texture_last_and_beyond, lambda r: r["stats"]["beyond_table"] > 0 and r["stats"]["taps"]["last"] > 0),
    "texture_nan_uv": (texture_nan_uv, lambda r: np.isnan(r["planes"][2]).any() and np.isfinite(r["planes"][2]).any() and r["stats"]["taps"]["nan"] > 0),
    "materials_and_normal_map": (materials_and_normal_map, lambda r: r["stats"]["materials"] == {0, 1} and (np.abs(r["planes"][1][r["covered"]][:, 0]) > 0.05).any()),
    "multiple_draws": (multiple_draws, lambda r: r["next_prim_base"] == 16 and len(r["stats"]["materials"]) == 3),
    "multiple_draws_high_prim_base": (multiple_draws_high_prim_base, lambda r: int((r["keys"] & np.uint64(0xFFFFFFFF)).max()) > 2 ** 32 - 8),
    "triangle_larger_than_the_frame": (triangle_larger_than_the_frame, lambda r: r["covered"].all() and r["stats"]["large"] >= 2),
    "empty_frame": (empty_frame, lambda r: not r["covered"].any()),
    "constant_material_quad": (constant_material_quad, lambda r: r["covered"].all()),
}
CULL_BACK_CASES = ("shared_edge_quad", "tie_coplanar_reversed_indices", "near_plane", "materials_and_normal_map")
# 72 x 40: three tile rows; the last is 200 x 136, 4 x 3 superblocks of a large triangle in bands whose first row is no multiple of 64
BAND_CASES = ("near_plane", "materials_and_normal_map", "grazing_quad", "triangle_larger_than_the_frame")
GOLDEN_CASES = ("near_plane", "instance_indirection", "texture_2x3_srgb")
NUM_SOUPS = 40


def with_cull_back(s):
    s = dict(s)
    s["draws"] = [dict(d, cull_back=True) for d in s["draws"]]
    return s


def prepass_depth(s, extra=None):
    """the depth prepass of the scene's own draws through the project's oracle (oracle.raster_depth, camera form); extra: a draw only the prepass sees"""
    from oracle import oracle
    depth = np.zeros((s["H"], s["W"]), f32)
    for d in list(s["draws"]) + ([extra] if extra is not None else []):
        if len(d["indices"]) == 0:
            continue
        first = d.get("first_instance", 0)
        nd = d["num_drawn"] if d.get("num_drawn") is not None else (len(d["instance_ids"]) if d["instance_ids"] is not None else len(s["instances"]) - first)
        ids = d["instance_ids"] if d["instance_ids"] is not None else np.arange(first, first + nd, dtype=np.uint32)
        depth = oracle.raster_depth(s["projection"], np.ascontiguousarray(d["vertices"][:, 2:5]), d["indices"], np.ascontiguousarray(s["instances"]["model"]), s["W"], s["H"],
                                    instance_ids=ids, depth=depth, view=s["view"], cull_back=d.get("cull_back", False))
    return depth


def prepass_only_draw(s):
    """geometry that only the prepass contains: a quad in front of everything over the frame's lower-right part"""
    if np.array_equal(s["projection"], screen_projection(s["W"], s["H"])):
        v, t = quad(s["W"] * 0.6, s["H"] * 0.55, s["W"] + 2.0, s["H"] + 2.0, z=0.95)
    else:
        v, t = quad(0.05, -0.9, 0.9, -0.05, z=-1.0)
        for q in v:
            q[4] = -1.02
    return draw(v, t, ids=[0])


# ---- a scene as flat arrays (the golden file's inputs) and back ---------------------------------------------------------------------------------------
def scene_to_arrays(s, prefix):
    out = {f"{prefix}.frame": np.array([s["W"], s["H"], s.get("prim_base", 0), len(s["draws"]), len(s["textures"])], np.int64),
           f"{prefix}.view": s["view"], f"{prefix}.projection": s["projection"], f"{prefix}.instances": s["instances"].view(np.uint8),
           f"{prefix}.materials": s["materials"].view(np.uint8), f"{prefix}.srgb": np.array(s["srgb"], np.uint8)}
    for k, t in enumerate(s["textures"]):
        out[f"{prefix}.texture{k}"] = t
    for k, d in enumerate(s["draws"]):
        out[f"{prefix}.draw{k}.vertices"], out[f"{prefix}.draw{k}.indices"] = d["vertices"], d["indices"]
        out[f"{prefix}.draw{k}.ids"] = d["instance_ids"] if d["instance_ids"] is not None else np.zeros(0, np.uint32)
        # has ids, firstInstance, numDrawn (-1: all), cull back
        out[f"{prefix}.draw{k}.params"] = np.array([d["instance_ids"] is not None, d["first_instance"], -1 if d["num_drawn"] is None else d["num_drawn"], d["cull_back"]], np.int64)
    return out


def scene_from_arrays(g, prefix):
    W, H, prim_base, nd, ntex = (int(x) for x in g[f"{prefix}.frame"])
    draws = []
    for k in range(nd):
        has_ids, first, num, cull = (int(x) for x in g[f"{prefix}.draw{k}.params"])
        draws.append(dict(vertices=g[f"{prefix}.draw{k}.vertices"], indices=g[f"{prefix}.draw{k}.indices"], instance_ids=g[f"{prefix}.draw{k}.ids"] if has_ids else None,
                          first_instance=first, num_drawn=None if num < 0 else num, cull_back=bool(cull)))
    return dict(W=W, H=H, view=g[f"{prefix}.view"], projection=g[f"{prefix}.projection"], instances=g[f"{prefix}.instances"].view(host.INSTANCE_DTYPE),
                materials=g[f"{prefix}.materials"].view(np.dtype(_lib.MATERIAL_DTYPE)), textures=[g[f"{prefix}.texture{k}"] for k in range(ntex)],
                srgb=[bool(b) for b in g[f"{prefix}.srgb"]], draws=draws, prim_base=prim_base)
