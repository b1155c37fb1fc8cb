"""The scenes of the indirect-draw tests (tests/test_indirect_cpu.py, tests/test_indirect_gpu.py): 96 x 64 frames (72 x 40 for the near-plane case) built
from the blocks of tests/surface_cases.py, tests/masked_cases.py and tests/gltf_cases.py.  A scene is the dict tests/indirect_ref.py describes: a draw with an
`indirect` entry is one command of DrawIndexedIndirect.  `records` is the numInstanceRecords the calls get; the instance buffer holds SLACK more records behind
it -- boxes right in front of the camera --, so that a wrong guard stays inside the allocation and shows in the picture.

CASES maps a name to (builder, predicate(expected result, decoded owners, scene)): what the case was built to reach, stated over the restatement.

CHAINS are the scenes of the cull -> draw chain: instance records with bounding spheres, the indirect commands as the host writes them (un-culled counts), a
frame from host.fill_frame_data that both the cull and the draws use, and the C oracle's survivor counts written down."""
import numpy as np

import gltf_cases as gc
import masked_cases as mc
import surface_cases as sc
from indirect_ref import drawn
from sailor_amd import host, synth
from surface_cases import FLAT_NORMAL, IDENTITY, WHITE, draw, material, scene, translation, vertex

f32 = np.float32
W, H = 96, 64
SLACK = 6


def indirect(d, capacity, count, first=0, records=None):
    d = dict(d, instance_ids=None, num_drawn=None, first_instance=0)
    d["indirect"] = dict(capacity=capacity, count=count, first=first, records=records)
    return d


def box_mesh():
    """the 12-triangle box of surface_cases.boxes_and_ground"""
    p, tris = synth.unit_cube_mesh()
    v = np.zeros((8, 18), f32)
    v[:, 2:5] = p; v[:, 0:2] = p[:, 0:2] * 0.5 + 0.5; v[:, 5:8] = p / np.sqrt(3); v[:, 8:11] = (1, 0, 0); v[:, 11:14] = (0, 1, 0); v[:, 14:18] = 1
    return v, tris


def box_models(n, seed=3):
    """n boxes on a 6-wide grid in front of the camera, overlapping their neighbours on the screen, every one at its own depth under its own rotation"""
    rng = np.random.default_rng(seed)
    return [host.transform_matrix([-4.5 + 1.8 * (k % 6), -2.7 + 1.8 * (k // 6), -6.0 - 0.3 * k, 1.0], (lambda q: q / np.linalg.norm(q))(rng.normal(size=4)),
                                  [0.8, 0.8, 0.8, 1.0]) for k in range(n)]


def slack_models():
    return [host.transform_matrix([-1.5 + 0.6 * k, 0.0, -2.5, 1.0], [0.0, 0.0, 0.0, 1.0], [0.5, 0.5, 0.5, 1.0]) for k in range(SLACK)]


def cam_quad(x0, y0, x1, y1, z, uv=((0, 0), (1, 0), (1, 1), (0, 1)), alpha=(1, 1, 1, 1)):
    p = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return [vertex((p[k][0], p[k][1], z), uv[k], (1, 1, 1, alpha[k])) for k in range(4)], [(0, 1, 2), (0, 2, 3)]


BOX_TEXTURES = dict(textures=[sc.distinct_texture(16, 16, 2), FLAT_NORMAL, sc.distinct_texture(8, 8, 3)], srgb=[True, False, True])
BOX_MATERIALS = [material(samplers=(0, 2, 1, 2)), material(albedo=(0.5, 0.7, 0.4, 1), samplers=(2, 0, 1, 0))]


def with_slack(s, records):
    """the scene's instance buffer followed by SLACK boxes no draw may reach; `records` is what the calls are told"""
    extra = sc.instances(slack_models(), [0] * SLACK)
    s["instances"] = np.concatenate([s["instances"].view(np.uint8).reshape(-1, 96), extra.view(np.uint8).reshape(-1, 96)]).reshape(-1).view(host.INSTANCE_DTYPE)
    s["records"] = records
    return s


def boxes(commands, backdrop=True, w=W, h=H):
    """24 box records, 2 backdrop records.  commands: (capacity, count, first, records) per box draw; then the backdrop quad, two instances of it, as a
    fully counted indirect draw behind everything: a following draw, ordered behind whatever the box draws counted"""
    v, t = box_mesh()
    draws = [indirect(draw(v, t, cull_back=True), *c) for c in commands]
    if backdrop:
        q, qt = cam_quad(-40.0, -25.0, 40.0, 25.0, -30.0, uv=((0, 0), (5, 0), (5, 3), (0, 3)))
        draws.append(indirect(draw(q, qt), 2, 2, 24, 26))
    models = box_models(24) + [IDENTITY, translation(3.0, 2.0, 1.0)]
    s = scene(w, h, sc.camera_projection(w, h, 0.5), draws, models=models, mats=BOX_MATERIALS, inst_materials=[k % 2 for k in range(24)] + [1, 0], **BOX_TEXTURES)
    return with_slack(s, 26)


def ground_quad():
    """a two-triangle ground quad, capacity 40 and count 3: 80 lanes, the first wave holds 6 live ones and 58 dead ones next to large triangles, and the slices
    chosen from the capacity are 256 -- the large-triangle path with dead lanes in the wave and gridDim.y > 1"""
    g = [vertex((-4, -2, -1), (0, 0)), vertex((4, -2, -1), (2, 0)), vertex((4, -2, -60), (2, 15)), vertex((-4, -2, -60), (0, 15))]
    models = [translation(-6.0 + 6.0 * (k % 3), 0.2 * k, 0.0) for k in range(40)]   # three strips side by side, two units of overlap, rising with k
    s = scene(W, H, sc.camera_projection(W, H, 0.5), [indirect(draw(g, [(0, 1, 2), (0, 2, 3)]), 40, 3)], models=models, mats=BOX_MATERIALS,
              inst_materials=[k % 2 for k in range(40)], **BOX_TEXTURES)
    return with_slack(s, 40)


def near_cut_partial():
    """surface_cases.near_plane (one vertex beyond the near plane, two beyond, one behind the eye) in five instances of which three are counted"""
    base = sc.near_plane()
    d = base["draws"][0]
    models = [translation(0.15 * k, -0.1 * k, -0.05 * k) for k in range(5)]
    s = scene(72, 40, sc.camera_projection(72, 40), [indirect(draw(d["vertices"], d["indices"]), 5, 3)], models=models)
    return with_slack(s, 5)


def _cutout_quads(n):
    """n instances of a checker quad, side by side with a little overlap, each a little farther; materials 2.. carry alpha textures"""
    q, t = cam_quad(-0.9, -0.9, 0.9, 0.9, 0.0, uv=((0, 0), (2, 0), (2, 2), (0, 2)), alpha=(1.0, 0.9, 0.8, 1.0))
    models = [translation(-4.0 + 1.6 * k, -1.0 + 0.5 * k, -5.0 - 0.2 * k) for k in range(n)]
    return q, t, models


CUTOUT_TEXTURES = dict(textures=[WHITE, FLAT_NORMAL, mc.checker(2), mc.checker(4), mc.alpha_texture([[255, 0, 255]]), mc.alpha_texture([[200, 100], [60, 255]])],
                       srgb=[False] * 6)


def cutout_partial():
    """a cutout draw over seven records, first 1, four of a capacity of six counted, four albedo samplers among them"""
    q, t, models = _cutout_quads(7)
    mats = [material(albedo=(k / 6 + 0.1, 1 - k / 6, 0.5, 1), samplers=(2 + k % 4, 0, 1, 0)) for k in range(4)]
    s = scene(W, H, sc.camera_projection(W, H, 0.5), [mc.cutout(indirect(draw(q, t), 6, 4, 1))], models=models, mats=mats, inst_materials=[k % 4 for k in range(7)],
              **CUTOUT_TEXTURES)
    return with_slack(s, 7)


def gltf_partial():
    """the same records drawn by Standard_glTF.shader: a cutout draw against the materials' alphaCutoff 0.3, and a plain glTF draw of boxes behind it, both
    partially counted"""
    q, t, models = _cutout_quads(7)
    v, bt = box_mesh()
    mats = [gc.gltf_material(base=(k / 6 + 0.1, 1 - k / 6, 0.5, 1), emissive=(0.2, 0.1, 0.3, 0), cutoff=0.3, samplers=(2 + k % 4, 1, 0, 0, 0)) for k in range(4)]
    boxes_ = [host.transform_matrix([-3.0 + 2.0 * k, 1.5, -8.0 - 0.3 * k, 1.0], [0.1, 0.3, 0.2, 0.927], [0.9, 0.9, 0.9, 1.0]) for k in range(4)]
    draws = [gc.gltf(indirect(draw(v, bt, cull_back=True), 4, 3, 7)), gc.gltf(mc.cutout(indirect(draw(q, t), 6, 4, 1)))]
    s = scene(W, H, sc.camera_projection(W, H, 0.5), draws, models=models + boxes_, mats=mats, inst_materials=[k % 4 for k in range(11)], **CUTOUT_TEXTURES)
    return with_slack(s, 11)


def mixed_direct_and_indirect():
    """direct draws (with instance ids, with firstInstance) and indirect ones in one pass, both shaders, with and without the cutout: a direct box draw, an
    indirect box draw (5 of 8), a direct Standard cutout draw, an indirect glTF cutout draw (2 of 3), a direct box draw behind an empty indirect one"""
    v, bt = box_mesh()
    q, t, quads = _cutout_quads(6)
    mats = BOX_MATERIALS + [material(samplers=(3, 0, 1, 0)), gc.gltf_material(base=(0.9, 0.6, 0.3, 1), emissive=(0.3, 0.2, 0.1, 0), cutoff=0.3, samplers=(5, 1, 0, 0, 0))]
    models = box_models(16) + quads                       # records 0..15 boxes, 16..18 Standard quads, 19..21 glTF quads
    draws = [draw(v, bt, ids=[3, 1, 4], cull_back=True),
             indirect(draw(v, bt, cull_back=True), 8, 5, 8),
             mc.cutout(draw(q, t, first_instance=16, num_drawn=3)),
             gc.gltf(mc.cutout(indirect(draw(q, t), 3, 2, 19))),
             indirect(draw(v, bt), 4, 0, 0),
             draw(v, bt, first_instance=5, num_drawn=2)]
    s = scene(W, H, sc.camera_projection(W, H, 0.5), draws, models=models, mats=mats, inst_materials=[k % 2 for k in range(16)] + [2] * 3 + [3] * 3,
              textures=[sc.distinct_texture(16, 16, 2), FLAT_NORMAL, sc.distinct_texture(8, 8, 3), mc.checker(4), WHITE, mc.alpha_texture([[200, 100], [60, 255]])],
              srgb=[True, False, True, False, False, False])
    return with_slack(s, 22)


def _counts(s):
    return [drawn(d["indirect"], s["records"]) for d in s["draws"] if d.get("indirect") is not None]


def _slots(o):
    return set(int(x) for x in np.unique(o["slot"])) - {-1}


def _instances_of(o, slot):
    return set(int(x) for x in np.unique(o["d"][o["slot"] == slot]))


def _box_case(count, capacity=24, first=0, records=None, want=None):
    want = count if want is None else want
    return (lambda: boxes([(capacity, count, first, records)]),
            lambda r, o, s: _counts(s) == [want, 2] and _slots(o) == ({0, 1} if want else {1}) and (want == 0 or max(_instances_of(o, 0)) == want - 1))


CASES = {
    # 60 / 72 / 252 / 264 lanes of 288: across a wave edge (64) and a block edge (256)
    "boxes_5_of_24": _box_case(5),
    "boxes_6_of_24": _box_case(6),
    "boxes_21_of_24": _box_case(21),
    "boxes_22_of_24": _box_case(22),
    "count_0_and_a_following_draw": _box_case(0),
    "count_equals_capacity": _box_case(24),
    "count_above_capacity_is_clamped": _box_case(1000, capacity=20, want=20),
    "first_instance_7": _box_case(9, first=7),
    "first_plus_count_past_the_records": _box_case(10, first=20, records=24, want=4),
    "first_instance_at_and_beyond_the_records": (lambda: boxes([(24, 5, 24, 24), (24, 5, 0xFFFFFFF0, 24), (24, 0xFFFFFFFF, 0xFFFFFFFF, 26)]),
                                                 lambda r, o, s: _counts(s) == [0, 0, 0, 2] and _slots(o) == {3}),
    "ground_quad_3_of_40": (ground_quad, lambda r, o, s: _counts(s) == [3] and r["stats"]["large"] >= 3 and _instances_of(o, 0) == {0, 1, 2}),
    "near_cut_partial": (near_cut_partial, lambda r, o, s: _counts(s) == [3] and r["stats"]["cut_two"] >= 3 and (o["part"] == 1).any()
                         and len(_instances_of(o, 0)) == 3),
    "cutout_partial": (cutout_partial, lambda r, o, s: _counts(s) == [4] and r["stats"]["discarded"] > 50 and r["cutout"].sum() > 50 and len(_instances_of(o, 0)) == 4),
    "gltf_partial": (gltf_partial, lambda r, o, s: _counts(s) == [3, 4] and r["stats"]["discarded"] > 50 and (r["gltf"] & r["cutout"]).sum() > 50
                     and (r["gltf"] & ~r["cutout"]).sum() > 50),
    "mixed_direct_and_indirect": (mixed_direct_and_indirect, lambda r, o, s: _counts(s) == [5, 2, 0] and _slots(o) == {0, 1, 2, 3, 5}
                                  and (r["gltf"] & r["cutout"]).any() and (~r["gltf"] & r["cutout"]).any()),
}
BAND_CASES = ("boxes_21_of_24", "ground_quad_3_of_40", "gltf_partial", "mixed_direct_and_indirect")   # 96 x 64: four tile rows


def all_scenes():
    return {name: build() for name, (build, _) in CASES.items()}


def prepass(s):
    """DepthPrepass Opaque, then Masked, over the draws that draw something (the survivors scene)"""
    live = dict(s, draws=[d for d in s["draws"] if d.get("num_drawn") != 0])
    return gc.full_prepass(live)


# ---- the cull -> draw chain -------------------------------------------------------------------------------------------------------------------------
def chain_frame():
    """identity camera, fov 90, near 1, far 20000, 96 x 64: the frame of the cull AND of the draws"""
    world = host.transform_matrix([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0])
    return host.fill_frame_data(world, 90.0, 1.0, 20000.0, W, H)


def _sphere(inst, radius):
    inst["sphereBounds"][:, :3] = 0.0
    inst["sphereBounds"][:, 3] = radius
    return inst


def _chain_scene(frame, draws, models, inst_materials, radii, batches):
    s = scene(W, H, np.array(frame.projection, f32), draws, models=models, view=np.array(frame.view, f32), mats=BOX_MATERIALS, inst_materials=inst_materials,
              **BOX_TEXTURES)
    s["instances"]["sphereBounds"][:, 3] = radii
    n = len(models)
    s = with_slack(s, n)
    s["instances"]["sphereBounds"][n:, 3] = 1.0
    b = np.zeros((len(batches), 5), np.uint32)
    for k, (nt, count, first) in enumerate(batches):
        b[k] = (3 * nt, count, 0, 0, first)
    return dict(scene=s, frame=frame, batches=b)


def chain_frustum():
    """24 box records, every third one far outside the view (to the left, to the right, behind the camera in turn), then 4 quad records of which the middle
    two are outside: two commands.  Every sphere is many radii away from every plane."""
    v, bt = box_mesh()
    inside = box_models(24, seed=9)
    out_at = [(-400.0, 0.0, -20.0), (400.0, 30.0, -20.0), (0.0, 0.0, 300.0)]
    models = [inside[k] if k % 3 != 1 else host.transform_matrix([*out_at[(k // 3) % 3], 1.0], [0.0, 0.0, 0.0, 1.0], [0.8, 0.8, 0.8, 1.0]) for k in range(24)]
    q, t = cam_quad(-1.0, -1.0, 1.0, 1.0, 0.0, uv=((0, 0), (2, 0), (2, 2), (0, 2)))
    quads = [translation(-2.0, 1.0, -4.0), translation(0.0, 900.0, -10.0), translation(0.0, -900.0, -10.0), translation(2.0, -1.0, -4.5)]
    draws = [indirect(draw(v, bt, cull_back=True), 24, 24, 0), indirect(draw(q, t), 4, 4, 24)]
    return _chain_scene(chain_frame(), draws, models + quads, [k % 2 for k in range(28)], [np.sqrt(3.0)] * 24 + [1.5] * 4, [(12, 24, 0), (2, 4, 24)])


def chain_frustum_turned():
    """the same layout with other records inside: what the second replay of the captured chain is given"""
    c = chain_frustum()
    m = c["scene"]["instances"]["model"]
    m[0:24] = np.roll(m[0:24], 1, axis=0)      # the outside boxes are now every third one from record 2
    m[[24, 25]] = m[[25, 24]]                 # the first quad is outside, the second inside
    return c


def chain_occlusion():
    """a wall over the whole view at z = -5 (its bounding sphere reaches the near plane: ProjectSphere's gate keeps it), twelve boxes between z = -40 and
    z = -51 behind it: with the pyramid of the wall's depth every box is occluded"""
    v, bt = box_mesh()
    wall, wt = cam_quad(-12.0, -8.0, 12.0, 8.0, 0.0, uv=((0, 0), (4, 0), (4, 3), (0, 3)))
    models = [translation(0.0, 0.0, -5.0)] + [host.transform_matrix([-5.0 + 2.0 * (k % 6), -1.0 + 2.0 * (k // 6), -40.0 - k, 1.0], [0.0, 0.0, 0.0, 1.0],
                                                                     [0.8, 0.8, 0.8, 1.0]) for k in range(12)]
    draws = [indirect(draw(wall, wt), 1, 1, 0), indirect(draw(v, bt, cull_back=True), 12, 12, 1)]
    c = _chain_scene(chain_frame(), draws, models, [1] + [0] * 12, [15.0] + [np.sqrt(3.0)] * 12, [(2, 1, 0), (12, 12, 1)])
    c["hiz"] = (W // 2, W // 2, 5)     # DepthHighZ is ViewportWidth / 2 squared (DefaultRenderer.renderer)
    return c


# name -> (builder, the C oracle's instanceCount per command after the cull)
CHAINS = {
    "chain_frustum": (chain_frustum, [16, 2]),
    "chain_frustum_turned": (chain_frustum_turned, [16, 2]),
    "chain_occlusion": (chain_occlusion, [1, 0]),
}


def chain_after_cull(c, hiz=None):
    """the C oracle's cull + compaction over the chain's records -> (the scene with the compacted records and commands that hold the survivor counts, counts)"""
    from oracle import oracle
    s = c["scene"]
    n = s["records"]
    inst, batches = oracle.mesh_cull_compact(c["frame"], s["instances"][:n].copy(), n, 0, c["batches"].copy(), hiz=hiz)
    after = dict(s, instances=s["instances"].copy())
    after["instances"][:n] = inst
    counts = [int(x) for x in batches[:, 1]]
    k, draws = 0, []
    for d in s["draws"]:
        ind = dict(d["indirect"], count=counts[k], first=int(batches[k, 4]))
        draws.append(dict(d, indirect=ind))
        k += 1
    after["draws"] = draws
    return after, counts
