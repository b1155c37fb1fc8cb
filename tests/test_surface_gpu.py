"""RenderScene's surface pass (sailor_amd/csrc/surface.hip) through the C-ABI against tests/surface_ref.py: keys, depth and coverage bit for bit, the three
planes bit for bit with non-finite values compared by class -- every case of tests/surface_cases.py with and without a prepass, the bands, the golden file,
the refusals, 40 random soups, and one frame from entities to a composited Main."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import surface_cases as cases
import surface_ref as ref
from oracle import oracle
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import EcsSweep, ForwardPlus, SurfacePass, linearize_depth, upload_lights, upload_textures

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "tiny_surface.npz"


def frame_of(s):
    f = _lib.UboFrameData()
    f.view[:] = [float(x) for x in s["view"]]
    f.projection[:] = [float(x) for x in s["projection"]]
    f.viewportSize[:] = [s["W"], s["H"]]
    return f


def dev(ctx, a, view=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view is not None else a).to(ctx.device)


class Uploaded:
    """a scene's buffers on the device"""

    def __init__(self, ctx, s):
        self.s, self.frame = s, frame_of(s)
        self.instances = dev(ctx, s["instances"].view(np.uint8))
        self.materials = dev(ctx, s["materials"].view(np.uint8))
        self.textures, self.num_textures, self.keep = upload_textures(ctx, s["textures"], s["srgb"])
        self.draws = [(dev(ctx, d["vertices"]), dev(ctx, d["indices"], np.int32) if len(d["indices"]) else torch.zeros(3, dtype=torch.int32, device=ctx.device),
                       None if d["instance_ids"] is None else dev(ctx, d["instance_ids"], np.int32), d) for d in s["draws"]]


def run(ctx, s, prepass=None, band=None, up=None):
    """the scene through begin / draw / resolve -> dict like surface_ref.render's"""
    up = up or Uploaded(ctx, s)
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=max(len(s["draws"]), 1))
    sp.begin(None if prepass is None else dev(ctx, prepass), prim_base=s.get("prim_base", 0))
    for v, i, ids, d in up.draws:
        sp.draw(up.frame, v, i if len(d["indices"]) else i[:0], up.instances, ids, num_drawn=d["num_drawn"], first_instance=d["first_instance"], cull_back=d["cull_back"])
    surface, depth, cov = sp.resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures)
    keys = sp.download_keys()
    return dict(planes=surface.cpu().numpy(), depth=depth.cpu().numpy(), covered=cov.cpu().numpy().astype(bool), keys=keys, sp=sp, up=up)


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got["keys"], want["keys"], err_msg=f"{what}: keys")
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), err_msg=f"{what}: depth")
    np.testing.assert_array_equal(got["covered"], want["covered"], err_msg=f"{what}: coverage")
    same = ref.same_bits_or_class(got["planes"], want["planes"])
    assert same.all(), f"{what}: {(~same).sum()} plane words differ, first at {np.argwhere(~same)[:4].tolist()}"


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_against_the_restatement_with_and_without_a_prepass(ctx, name):
    s = cases.CASES[name][0]()
    up = Uploaded(ctx, s)
    want = ref.render(s)
    assert_same(run(ctx, s, up=up), want, name)
    pre = cases.prepass_depth(s)
    assert_same(run(ctx, s, prepass=pre, up=up), ref.render(s, prepass=pre), f"{name} behind its prepass")
    if name in cases.CULL_BACK_CASES:
        c = cases.with_cull_back(s)
        assert_same(run(ctx, c), ref.render(c), f"{name} with back-face culling")


def test_depth_output_is_the_depth_prepass_of_the_gpu(ctx):
    """the final depth of the pass == sailor_hip_raster_depth_camera over the same draws, bit for bit"""
    lib = ctx._lib
    for name in ("near_plane", "materials_and_normal_map", "multiple_draws", "triangle_larger_than_the_frame", "degenerates"):
        s = cases.CASES[name][0]()
        got = run(ctx, s)
        W, H = s["W"], s["H"]
        depth = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
        models = dev(ctx, np.ascontiguousarray(s["instances"]["model"]))
        keep = []
        for d in s["draws"]:
            first = d["first_instance"]
            nd = d["num_drawn"] if d["num_drawn"] is not None else (len(d["instance_ids"]) if d["instance_ids"] is not None else len(s["instances"]) - first)
            ids = d["instance_ids"] if d["instance_ids"] is not None else np.arange(first, first + nd, dtype=np.uint32)
            pos, idx, dids = dev(ctx, np.ascontiguousarray(d["vertices"][:, 2:5])), dev(ctx, d["indices"], np.int32), dev(ctx, ids, np.int32)
            keep += [pos, idx, dids]
            _lib.check(lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(got["up"].frame), pos.data_ptr(), idx.data_ptr(), len(d["indices"]), models.data_ptr(),
                                                          dids.data_ptr(), nd, W, H, depth.data_ptr(), 0, None), "sailor_hip_raster_depth_camera", ctx.handle)
        ctx.synchronize()
        np.testing.assert_array_equal(got["depth"].view(np.uint32), depth.cpu().numpy().view(np.uint32), err_msg=name)


def test_a_prepass_with_geometry_the_scene_does_not_draw(ctx):
    for name in ("multiple_draws", "near_plane"):
        s = cases.CASES[name][0]()
        both = cases.prepass_depth(s, cases.prepass_only_draw(s))
        got, want = run(ctx, s, prepass=both), ref.render(s, prepass=both)
        assert_same(got, want, name)
        hidden = both != cases.prepass_depth(s)
        assert hidden.sum() > 20 and not got["covered"][hidden].any()
        np.testing.assert_array_equal(got["depth"].view(np.uint32), both.view(np.uint32))


def test_bands_concatenate_to_the_whole_frame(ctx):
    for name in cases.BAND_CASES:
        s = cases.CASES[name][0]()
        up, whole = Uploaded(ctx, s), ref.render(s)
        pre = cases.prepass_depth(s)
        for world in (2, 3):
            parts = []
            for rank in reversed(range(world)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
                band = host.band_for_rank(s["W"], s["H"], rank, world)
                got = run(ctx, s, prepass=pre if world == 3 else None, band=band, up=up)
                assert_same(got, ref.render(s, prepass=pre if world == 3 else None, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)), f"{name} band {rank}/{world}")
                parts.append(got)
            np.testing.assert_array_equal(np.concatenate([p["keys"] for p in parts]), whole["keys"])
            assert ref.same_bits_or_class(np.concatenate([p["planes"] for p in parts], axis=1), whole["planes"]).all()


def test_golden_through_the_c_abi(ctx):
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        got = run(ctx, cases.scene_from_arrays(g, name))   # inputs from the file alone
        np.testing.assert_array_equal(got["keys"], g[f"{name}.keys"])
        assert ref.same_bits_or_class(got["planes"], g[f"{name}.planes"]).all()


def test_random_soups(ctx):
    reached = dict(cut_one=0, cut_two=0, beyond_table=0, overwritten=0)
    for seed in range(cases.NUM_SOUPS):
        s = cases.random_soup(seed)
        want = ref.render(s)
        assert_same(run(ctx, s), want, f"soup {seed}")
        for k in reached:
            reached[k] += want["stats"][k]
    assert all(v > 0 for v in reached.values()), reached


def test_refusals_launch_nothing_and_say_why(ctx):
    lib = ctx._lib
    s = cases.multiple_draws()
    W, H = s["W"], s["H"]
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, W, H, max_draws=2)
    sp.begin()
    ws, n = sp.workspace.data_ptr(), sp.workspace.numel()
    band, frame = sp.band, up.frame
    v, i, ids, d = up.draws[0]
    bad_band = _lib.Band(0, 1, 3, 16)
    surface = torch.empty((3, H, W, 4), dtype=torch.float32, device=ctx.device)
    target = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)

    def desc(prim_base=0, vertices=v.data_ptr(), flags=0):
        return _lib.SurfaceDraw(vertices, i.data_ptr(), ids.data_ptr(), len(d["indices"]), len(d["instance_ids"]), prim_base, flags, 0, 0)

    def draw_call(dd, index=0, workspace=ws, size=n, b=band, inst=up.instances.data_ptr()):
        return lambda: lib.sailor_hip_surface_draw(ctx.handle, C.byref(frame), C.byref(dd), inst, index, W, H, C.byref(b), workspace, size)

    def resolve_call(workspace=ws, size=n, b=band, out=surface.data_ptr(), stride=H * W, mats=up.materials.data_ptr(), tex=up.textures.data_ptr(), inst=up.instances.data_ptr()):
        return lambda: lib.sailor_hip_surface_resolve(ctx.handle, C.byref(frame), inst, mats, len(s["materials"]), tex, up.num_textures, W, H, C.byref(b), workspace, size, out,
                                                      stride, None, None)
    assert lib.sailor_hip_surface_workspace_bytes(W, H, C.byref(bad_band), 2) == 0 and lib.sailor_hip_surface_workspace_bytes(W, H, C.byref(band), 0) == 0
    misuse = {
        "begin: null workspace": lambda: lib.sailor_hip_surface_begin(ctx.handle, None, W, H, C.byref(band), None, n),
        "begin: workspace too small": lambda: lib.sailor_hip_surface_begin(ctx.handle, None, W, H, C.byref(band), ws, lib.sailor_hip_surface_keys_offset() + W * H * 8),
        "begin: invalid band": lambda: lib.sailor_hip_surface_begin(ctx.handle, None, W, H, C.byref(bad_band), ws, n),
        "draw: null vertices": draw_call(desc(vertices=None)),
        "draw: null instances": draw_call(desc(), inst=None),
        "draw: null workspace": draw_call(desc(), workspace=None),
        "draw: workspace too small": draw_call(desc(), size=1000),
        "draw: drawIndex >= maxDraws": draw_call(desc(), index=2),
        "draw: primBase overflow": draw_call(desc(prim_base=2 ** 32 - 1 - 8)),   # 8 primitives: the last order + 1 would be 2^32 - 1 + ... past the word
        "draw: unknown flags": draw_call(desc(flags=2)),
        "draw: invalid band": draw_call(desc(), b=bad_band),
        "resolve: null surface": resolve_call(out=None),
        "resolve: null materials": resolve_call(mats=None),
        "resolve: null textures": resolve_call(tex=None),
        "resolve: planeStride too small": resolve_call(stride=H * W - 1),
        "resolve: workspace too small": resolve_call(size=1000),
        "resolve: invalid band": resolve_call(b=bad_band),
        "composite: null radiance": lambda: lib.sailor_hip_surface_composite(ctx.handle, None, ws, n, target.data_ptr(), W, H, C.byref(band)),
        "composite: null target": lambda: lib.sailor_hip_surface_composite(ctx.handle, target.data_ptr(), ws, n, None, W, H, C.byref(band)),
        "composite: invalid band": lambda: lib.sailor_hip_surface_composite(ctx.handle, target.data_ptr(), ws, n, target.data_ptr(), W, H, C.byref(bad_band)),
    }
    for what, call in misuse.items():
        before, _ = ctx.launch_log(0)
        assert call() == -1, what
        after, _ = ctx.launch_log(0)
        assert after == before, f"{what}: launched {after - before} kernels"
        assert b"sailor_hip_surface_" in lib.sailor_hip_context_last_error(ctx.handle), what
    # the largest primBase that is still accepted: the draw's last order + 1 is 2^32 - 2
    assert draw_call(desc(prim_base=2 ** 32 - 2 - 8))() == 0
    ctx.synchronize()
    # the kernels of one pass, by name
    names = ctx.launches_of(lambda: (sp.begin(), sp.draw(frame, v, i, up.instances, ids), sp.resolve(frame, up.instances, up.materials, up.textures, up.num_textures),
                                     sp.composite(target.clone(), target)))
    assert names == ["k_surface_begin", "k_surface_visibility", "k_surface_resolve", "k_surface_composite"], names
    ctx.synchronize()


def test_entities_to_a_composited_main(ctx):
    """entities -> ECS sweep -> depth prepass -> surface pass -> linearize -> light cull -> shade -> composite over a sky-coloured target, 96 x 64: covered
    pixels against the C oracle's shade of the RESTATEMENT's surface at the radiance bound (1e-4 relative), uncovered pixels keep the target bit for bit."""
    from sailor_amd.forward_plus import raster_depth_camera
    W, H = 96, 64
    f = synth.make_frame("tiny", with_surface=False, width=W, height=H)
    cam = f.cam
    ents = synth.make_entities(500)
    ents.transforms[:, 0:3] *= np.float32(0.12)
    planes, _ = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)
    world, aabb, vis = EcsSweep(ctx, ents).run(planes)
    ids = np.nonzero(np.unpackbits(vis.cpu().numpy().view(np.uint8), bitorder="little")[:500])[0].astype(np.uint32)[:96]
    assert len(ids) >= 32
    box = cases.boxes_and_ground(1, W, H)["draws"][0]
    models = synth.caster_models(world.cpu().numpy(), ents.local_aabb)
    fb = np.frombuffer(bytes(cam.frame), np.float32)
    rng = np.random.default_rng(3)
    s = cases.scene(W, H, fb[16:32].copy(), [cases.draw(box["vertices"], box["indices"], ids=ids, cull_back=True)], models=models, view=fb[0:16].copy(),
                    textures=[cases.distinct_texture(16, 16, 2), cases.FLAT_NORMAL, cases.distinct_texture(4, 4, 5)], srgb=[True, False, False],
                    mats=[cases.material(albedo=(0.9, 0.8, 0.7, 1), metallic=0.3, roughness=0.6, samplers=(0, 2, 1, 2)),
                          cases.material(albedo=(0.4, 0.6, 0.9, 1), metallic=0.8, roughness=0.3, samplers=(2, 0, 1, 0))], inst_materials=rng.integers(0, 2, len(models)))
    up = Uploaded(ctx, s)
    d_pos = dev(ctx, np.ascontiguousarray(box["vertices"][:, 2:5]))
    raw = raster_depth_camera(ctx, cam.frame, d_pos, up.draws[0][1], dev(ctx, models), W, H, up.draws[0][2], cull_back=True)
    sp = SurfacePass(ctx, W, H)
    sp.begin(raw)
    sp.draw(cam.frame, up.draws[0][0], up.draws[0][1], up.instances, up.draws[0][2], cull_back=True)
    surface, depth, cov = sp.resolve(cam.frame, up.instances, up.materials, up.textures, up.num_textures)
    lin = linearize_depth(ctx, cam.frame, depth)
    fp = ForwardPlus(ctx, W, H, len(f.lights))
    lights = upload_lights(f.lights, ctx.device)
    fp.cull(cam.frame, lights, len(f.lights), lin)
    rad = torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device)   # through sailor_hip_shade_ex, over the canonical lists the cull packed
    _lib.check(ctx._lib.sailor_hip_shade_ex(ctx.handle, C.byref(cam.frame), surface.data_ptr(), H * W, lights.data_ptr(), len(f.lights), fp.grid.data_ptr(),
                                            fp.culled.data_ptr(), None, None, rad.data_ptr(), C.byref(fp.band), None), "sailor_hip_shade_ex", ctx.handle)
    sky = torch.from_numpy(rng.uniform(0, 1, (H, W, 4)).astype(np.float32)).to(ctx.device)
    main = sp.composite(rad, sky.clone()).cpu().numpy()
    ctx.synchronize()
    # the reference side: restatement -> oracle
    want = ref.render(s)
    np.testing.assert_array_equal(raw.cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))
    assert ref.same_bits_or_class(surface.cpu().numpy(), want["planes"]).all()
    c = want["covered"]
    np.testing.assert_array_equal(cov.cpu().numpy().astype(bool), c)
    assert 0.1 < c.mean() < 0.98, c.mean()
    og, oi, _ = oracle.light_cull(cam.frame, W, H, f.lights, oracle.linearize_depth(cam.frame.cameraZNearZFar[0], want["depth"]))
    orad = oracle.shade(cam.frame, W, H, want["planes"], f.lights, og, oi, None)
    err = np.abs(main[c].astype(np.float64) - orad[c])
    assert (err <= 1e-4 * np.abs(orad[c])).all(), err.max()
    assert orad[c][:, :3].max() > 0.01, "the covered pixels are lit"
    np.testing.assert_array_equal(main[~c].view(np.uint32), sky.cpu().numpy()[~c].view(np.uint32))


def test_launch_times_at_4k(ctx):
    """prints the per-launch medians at 3840 x 2160 -- 1 024 boxes (back faces culled) and a ground quad behind their depth prepass -- and the resolve's byte
    floor; asserts only that the launches happened (there is no parent to compare against)"""
    W, H = 3840, 2160
    s = cases.boxes_and_ground(1024, W, H)
    up = Uploaded(ctx, s)
    lib = ctx._lib
    models = dev(ctx, np.ascontiguousarray(s["instances"]["model"]))
    raw = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
    keep = []
    for d in s["draws"]:
        pos, idx = dev(ctx, np.ascontiguousarray(d["vertices"][:, 2:5])), dev(ctx, d["indices"], np.int32)
        dids = dev(ctx, np.arange(d["first_instance"], d["first_instance"] + d["num_drawn"], dtype=np.uint32), np.int32)
        keep += [pos, idx, dids]
        _lib.check(lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(up.frame), pos.data_ptr(), idx.data_ptr(), len(d["indices"]), models.data_ptr(), dids.data_ptr(),
                                                      d["num_drawn"], W, H, raw.data_ptr(), _lib.RASTER_CULL_BACK if d["cull_back"] else 0, None), "prepass", ctx.handle)
    sp = SurfacePass(ctx, W, H)
    radiance = torch.rand((H, W, 4), dtype=torch.float32, device=ctx.device)
    target = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    times = {"begin": [], "draw boxes": [], "draw ground": [], "resolve": [], "composite": []}
    for it in range(7):
        ctx.time_launches(0, 5)
        sp.begin(raw)
        for v, i, ids, d in up.draws:
            sp.draw(up.frame, v, i, up.instances, ids, num_drawn=d["num_drawn"], first_instance=d["first_instance"], cull_back=d["cull_back"])
        surface, depth, cov = sp.resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures)
        sp.composite(radiance, target)
        ctx.synchronize()
        if it >= 2:
            for slot, key in enumerate(times):
                times[key].append(ctx.timed_launch_ms(slot))
    covered = float(cov.float().mean())
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), raw.cpu().numpy().view(np.uint32))
    for key, v in times.items():
        print(f"surface launch {key} 3840x2160: median {np.median(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, n={len(v)})")
    floor = W * H * (8 + 48 + 4 + 1)   # the resolve reads a key and writes three float4, a depth and a coverage byte per pixel
    print(f"surface resolve 3840x2160: {covered:.3f} of the frame covered; byte floor {floor / 1e6:.1f} MB = {floor / 6.29e12 * 1e6:.1f} us at 6.29 TB/s")
    assert all(len(v) == 5 for v in times.values()) and covered > 0.3
