"""RenderScene's real draws through the C++ host mirror: a RenderScene node WITHOUT a `surface` resource and with batches in the scene view records
BeginRenderPass / BindMaterial / BindShaderBindings / BindVertexBuffer / BindIndexBuffer / DrawIndexed / EndRenderPass, and the HIP backend turns them into the
surface pass (begin, draw per batch, resolve, shade, composite): `Main` equals the C-ABI sequence bit for bit, with firstIndex, vertexOffset and
firstInstance all above 0.  With a `surface` resource the graph launches what it launched before; a missing binding refuses the frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import surface_cases as cases
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import ForwardPlus, HipContext, PreparedLights, SurfacePass, linearize_depth, upload_lights, upload_textures
from sailor_amd.runtime_binding import Runtime

pytestmark = pytest.mark.gpu
PAD_VERTICES, PAD_INDICES, PAD_INSTANCES = 4, 3, 2
NUM_BOXES = 48


def build():
    """a pool of two meshes behind padding (a box and a ground quad), instances behind two unused ones, two batches"""
    f = synth.make_frame("tiny", with_surface=False)
    rng = np.random.default_rng(21)
    box = cases.boxes_and_ground(1, f.cam.width, f.cam.height)
    cube, ground = box["draws"][0], box["draws"][1]
    gv = ground["vertices"].copy()
    gv[:, 2:5] = [(-400, 60, 100), (400, 60, 100), (400, 60, -900), (-400, 60, -900)]
    vertices = np.concatenate([np.zeros((PAD_VERTICES, 18), np.float32), cube["vertices"], gv])
    indices = np.concatenate([np.zeros(PAD_INDICES, np.uint32), cube["indices"].reshape(-1), ground["indices"].reshape(-1)]).astype(np.uint32)
    models = [cases.IDENTITY] * PAD_INSTANCES
    models += [host.transform_matrix([rng.uniform(-150, 150), rng.uniform(70, 230), rng.uniform(-400, -60), 1.0], (lambda q: q / np.linalg.norm(q))(rng.normal(size=4)),
                                     [*rng.uniform(8, 30, 3), 1.0]) for _ in range(NUM_BOXES)]
    models += [cases.IDENTITY]
    inst = cases.instances(models, rng.integers(0, 2, len(models)))
    mats = np.concatenate([cases.material(albedo=(0.9, 0.8, 0.7, 1), metallic=0.3, roughness=0.6, samplers=(0, 2, 1, 2)),
                           cases.material(albedo=(0.4, 0.6, 0.9, 1), metallic=0.8, roughness=0.3, samplers=(2, 0, 1, 0))])
    textures, srgb = [cases.distinct_texture(16, 16, 2), cases.FLAT_NORMAL, cases.distinct_texture(4, 4, 5)], [True, False, False]
    batches = np.uint32([[36, NUM_BOXES, PAD_INDICES, PAD_VERTICES, PAD_INSTANCES], [6, 1, PAD_INDICES + 36, PAD_VERTICES + 8, PAD_INSTANCES + NUM_BOXES]])
    return f, vertices, indices, inst, mats, textures, srgb, batches


class Scene:
    def __init__(self, ctx):
        self.f, vertices, indices, inst, mats, textures, srgb, self.batches = build()
        dev = ctx.device
        self.W, self.H = self.f.cam.width, self.f.cam.height
        self.vertices, self.indices = torch.from_numpy(vertices).to(dev), torch.from_numpy(indices.view(np.int32)).to(dev)
        self.instances, self.materials = torch.from_numpy(inst.view(np.uint8).copy()).to(dev), torch.from_numpy(mats.view(np.uint8).copy()).to(dev)
        self.textures, self.num_textures, self.keep = upload_textures(ctx, textures, srgb)
        self.lights = upload_lights(self.f.lights, dev)
        # the depth prepass of the same batches (DepthOnly.shader, back faces culled), and its linearised form for the light cull
        self.raw = torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)
        positions = torch.from_numpy(np.ascontiguousarray(vertices[:, 2:5])).to(dev)
        models = torch.from_numpy(np.ascontiguousarray(inst["model"])).to(dev)
        for count, n, first_index, vertex_offset, first_instance in self.batches.tolist():
            _lib.check(ctx._lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(self.f.cam.frame), positions.data_ptr() + 12 * vertex_offset, self.indices.data_ptr() + 4 * first_index,
                                                               count // 3, models.data_ptr() + 64 * first_instance, None, n, self.W, self.H, self.raw.data_ptr(),
                                                               _lib.RASTER_CULL_BACK, None), "sailor_hip_raster_depth_camera", ctx.handle)
        self.linear = linearize_depth(ctx, self.f.cam.frame, self.raw)
        self.sky = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (self.H, self.W, 4)).astype(np.float32)).to(dev)
        ctx.synchronize()

    def through_the_c_abi(self, ctx):
        """-> (Main float32 [H, W, 4], coverage bool [H, W])"""
        frame, n = self.f.cam.frame, len(self.f.lights)
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(self.raw)
        for count, drawn, first_index, vertex_offset, first_instance in self.batches.tolist():
            sp.draw(frame, self.vertices[vertex_offset:], self.indices[first_index:first_index + count], self.instances, None, num_drawn=drawn, first_instance=first_instance,
                    cull_back=True)
        surface, _, cov = sp.resolve(frame, self.instances, self.materials, self.textures, self.num_textures)
        fp = ForwardPlus(ctx, self.W, self.H, n, prepared=PreparedLights(ctx, self.lights, n))
        fp.cull(frame, self.lights, n, self.linear)
        main = sp.composite(fp.shade(frame, surface, self.lights, n), self.sky.clone())
        ctx.synchronize()
        return main.cpu().numpy(), cov.cpu().numpy().astype(bool)

    def runtime(self, with_scene=True, instances=True):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.build_graph(["LightCulling", "RenderScene"])
        rt.set_camera(self.f.cam)
        rt.set_lights(self.f.lights)
        rt.set_depth(self.linear)
        if with_scene:
            rt.set_scene(self.vertices, self.indices, self.instances if instances else None, self.materials, self.textures, self.num_textures, self.batches)
        return rt


@pytest.fixture(scope="module")
def scene(ctx):
    return Scene(ctx)


def frame_launches(rt):
    before, _ = rt.launch_log(0)
    status = rt.process_frame()
    rt.wait_idle()
    after, names = rt.launch_log(16)
    n = after - before
    assert n <= 16
    return status, names[len(names) - n:] if n else []


def test_main_through_the_runtime_equals_the_c_abi_sequence(ctx, scene):
    want, covered = scene.through_the_c_abi(ctx)
    assert 0.3 < covered.mean() < 0.99 and (want[covered][:, :3] > 0).any()
    rt = scene.runtime()
    try:
        main = scene.sky.clone()
        rt.set_scene_targets(main, scene.raw)
        status, names = frame_launches(rt)
        assert status == 0, status
        own = [n for n in names if n.startswith("k_surface")]
        assert own == ["k_surface_begin", "k_surface_visibility", "k_surface_visibility", "k_surface_resolve", "k_surface_composite"], names
        assert names[-1] == "k_surface_composite" and names.index("k_surface_resolve") < len(names) - 2, names   # the shade sits between resolve and composite
        torch.cuda.synchronize()
        got = main.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(got[~covered].view(np.uint32), scene.sky.cpu().numpy()[~covered].view(np.uint32))
        assert rt.process_frame() == 0   # a second frame reuses the driver's workspace and planes
        rt.wait_idle()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        rt.close()


def test_with_a_surface_resource_the_graph_launches_what_it_launched_before(ctx, scene):
    surface = torch.from_numpy(synth.make_frame("tiny").surface).to(ctx.device)
    logs = []
    for with_scene in (False, True):
        rt = scene.runtime(with_scene=with_scene)
        try:
            radiance = torch.zeros((scene.H, scene.W, 4), dtype=torch.float32, device=ctx.device)
            rt.set_surface(surface, radiance)
            if with_scene:
                rt.set_scene_targets(scene.sky.clone(), scene.raw)
            status, names = frame_launches(rt)
            assert status == 0
            logs.append((names, radiance.cpu().numpy()))
        finally:
            rt.close()
    assert logs[0][0] == logs[1][0] and not any(n.startswith("k_surface") for n in logs[1][0]), logs
    np.testing.assert_array_equal(logs[0][1].view(np.uint32), logs[1][1].view(np.uint32))


def test_a_missing_binding_refuses_the_frame(ctx, scene):
    rt = scene.runtime(instances=False)   # no per-instance SSBO `data`
    try:
        main = scene.sky.clone()
        rt.set_scene_targets(main, scene.raw)
        status, names = frame_launches(rt)
        assert status == -1 and not any(n.startswith("k_surface") for n in names), (status, names)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), scene.sky.cpu().numpy().view(np.uint32))
    finally:
        rt.close()
