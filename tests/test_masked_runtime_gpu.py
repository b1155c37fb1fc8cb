"""The Masked render queue through the C++ host mirror: two RenderScene nodes, `Tag: Opaque` then `Tag: Masked` as DefaultRenderer.renderer lists them, over a scene
of a ground, boxes and a checker-alpha quad whose batch is tagged Masked (ALPHA_CUTOUT, double-sided) through Runtime.set_scene_tags.  `Main` equals the C-ABI
sequence bit for bit, the depth attachment after the frame equals the masked prepass depth, and with no tags set the frame is what the untagged draws give
through sailor_hip_surface_draw -- the route of before the tags existed."""
import ctypes as C

import numpy as np
import pytest
import torch

import masked_cases
import surface_cases as cases
from sailor_amd import _lib, host
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, SurfacePass, linearize_depth, masked_depth_prepass, upload_lights, upload_textures
from sailor_amd.runtime_binding import Runtime
from test_surface_runtime_gpu import build

pytestmark = pytest.mark.gpu
BATCH_ALPHA_CUTOUT, BATCH_DOUBLE_SIDED = 1, 2


class Scene:
    """test_surface_runtime_gpu's pool (boxes and a ground behind padding) plus a quad with a 4 x 4 alpha checker, three batches"""

    def __init__(self, ctx):
        self.f, vertices, indices, inst, mats, textures, srgb, batches = build()
        dev = ctx.device
        self.W, self.H = self.f.cam.width, self.f.cam.height
        qv, qt = cases.quad(-1, -1, 1, 1, z=0.0, uv=((0, 0), (3, 0), (3, 3), (0, 3)))
        first_vertex, first_index, first_instance = len(vertices), len(indices), len(inst)
        vertices = np.concatenate([vertices, np.asarray(qv, np.float32)])
        indices = np.concatenate([indices, np.asarray(qt, np.uint32).reshape(-1)]).astype(np.uint32)
        models = list(inst["model"]) + [host.transform_matrix([0.0, 150.0, -200.0, 1.0], [0.0, 0.0, 0.0, 1.0], [150.0, 150.0, 150.0, 1.0])]
        inst = cases.instances(models, list(inst["materialInstance"]) + [2])
        mats = np.concatenate([mats, cases.material(albedo=(0.8, 0.9, 0.3, 1), metallic=0.1, roughness=0.7, samplers=(3, 2, 1, 2))])
        textures, srgb = textures + [masked_cases.checker(4)], srgb + [True]
        self.batches = np.concatenate([batches, np.uint32([[6, 1, first_index, first_vertex, first_instance]])])
        self.tags, self.flags = ["Opaque", "Opaque", "Masked"], [0, 0, BATCH_ALPHA_CUTOUT | BATCH_DOUBLE_SIDED]
        self.vertices, self.indices = torch.from_numpy(vertices).to(dev), torch.from_numpy(indices.view(np.int32)).to(dev)
        self.instances, self.materials = torch.from_numpy(inst.view(np.uint8).copy()).to(dev), torch.from_numpy(mats.view(np.uint8).copy()).to(dev)
        self.textures, self.num_textures, self.keep = upload_textures(ctx, textures, srgb)
        self.lights = upload_lights(self.f.lights, dev)
        frame = self.f.cam.frame
        # DepthPrepass `Tag: Opaque` (DepthOnly.shader, back faces culled), then `Tag: Masked` through the C-ABI: begin(opaque depth), the masked draw, store_depth
        self.opaque = torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)
        positions = torch.from_numpy(np.ascontiguousarray(vertices[:, 2:5])).to(dev)
        model_only = torch.from_numpy(np.ascontiguousarray(inst["model"])).to(dev)
        for count, n, fi, vo, fin in self.batches[:2].tolist():
            _lib.check(ctx._lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(frame), positions.data_ptr() + 12 * vo, self.indices.data_ptr() + 4 * fi, count // 3,
                                                               model_only.data_ptr() + 64 * fin, None, n, self.W, self.H, self.opaque.data_ptr(), _lib.RASTER_CULL_BACK, None),
                       "sailor_hip_raster_depth_camera", ctx.handle)
        self.raw = masked_depth_prepass(SurfacePass(ctx, self.W, self.H), frame, self.opaque.clone(), [self.draw_args(2)], self.instances, self.materials, self.textures,
                                        self.num_textures)
        self.linear = linearize_depth(ctx, frame, self.raw)
        self.sky = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (self.H, self.W, 4)).astype(np.float32)).to(dev)
        ctx.synchronize()

    def draw_args(self, k, cull_back=False):
        count, drawn, first_index, vertex_offset, first_instance = self.batches[k].tolist()
        return dict(vertices=self.vertices[vertex_offset:], indices=self.indices[first_index:first_index + count], instance_ids=None, num_drawn=drawn,
                    first_instance=first_instance, cull_back=cull_back)

    def one_pass(self, ctx, fp, main, depth, draws):
        """one RenderScene pass as the backend runs it: begin(depth), the draws, resolve, shade, composite, and the depth write if a cutout draw was among them"""
        frame, n = self.f.cam.frame, len(self.f.lights)
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(depth)
        for k, cutout, cull_back in draws:
            sp.draw(frame, instances=self.instances, alpha_cutout=cutout, materials=self.materials if cutout else None, textures=self.textures if cutout else None,
                    num_textures=self.num_textures if cutout else 0, **self.draw_args(k, cull_back))
        surface, _, cov = sp.resolve(frame, self.instances, self.materials, self.textures, self.num_textures)
        sp.composite(fp.shade(frame, surface, self.lights, n), main)
        if any(c for _, c, _ in draws):
            sp.store_depth(depth)
        return cov

    def through_the_c_abi(self, ctx, passes):
        """-> (Main, depth attachment after the frame, the passes' coverage)"""
        n = len(self.f.lights)
        fp = ForwardPlus(ctx, self.W, self.H, n, prepared=PreparedLights(ctx, self.lights, n))
        fp.cull(self.f.cam.frame, self.lights, n, self.linear)
        main, depth = self.sky.clone(), self.raw.clone()
        cov = [self.one_pass(ctx, fp, main, depth, draws).cpu().numpy().astype(bool) for draws in passes]
        ctx.synchronize()
        return main.cpu().numpy(), depth.cpu().numpy(), cov

    def runtime(self, nodes, tagged):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.build_graph(["LightCulling"] + nodes)
        rt.set_camera(self.f.cam)
        rt.set_lights(self.f.lights)
        rt.set_depth(self.linear)
        rt.set_scene(self.vertices, self.indices, self.instances, self.materials, self.textures, self.num_textures, self.batches)
        if tagged:
            rt.set_scene_tags(self.tags, self.flags)
        return rt


def frame_launches(rt):
    """-> (status, the names of the frame's launches -- of its last 16 if there were more: the driver's log keeps that many)"""
    before, _ = rt.launch_log(0)
    status = rt.process_frame()
    rt.wait_idle()
    after, names = rt.launch_log(16)
    n = min(after - before, 16)
    return status, names[len(names) - n:] if n else []


def surface_launches(names, expected):
    """the frame's k_surface_* launches are `expected` (as far back as the log reaches: at least its last six)"""
    own = [n for n in names if n.startswith("k_surface")]
    return len(own) >= min(6, len(expected)) and own == expected[len(expected) - len(own):]


@pytest.fixture(scope="module")
def scene(ctx):
    return Scene(ctx)


def test_the_masked_prepass_opened_the_checkers_holes(ctx, scene):
    opaque, raw = scene.opaque.cpu().numpy(), scene.raw.cpu().numpy()
    nearer = raw != opaque
    assert nearer.sum() > 300 and (raw[nearer] > opaque[nearer]).all()


def test_main_and_depth_through_two_tagged_nodes_equal_the_c_abi_sequence(ctx, scene):
    want, want_depth, (opaque_cov, masked_cov) = scene.through_the_c_abi(ctx, [[(0, False, True), (1, False, True)], [(2, True, False)]])
    assert opaque_cov.mean() > 0.3 and masked_cov.sum() > 300
    np.testing.assert_array_equal(want_depth.view(np.uint32), scene.raw.cpu().numpy().view(np.uint32))
    rt = scene.runtime(["RenderScene:Opaque", "RenderScene:Masked"], tagged=True)
    try:
        main, depth = scene.sky.clone(), scene.raw.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)
        assert status == 0, status
        assert surface_launches(names, ["k_surface_begin", "k_surface_visibility", "k_surface_visibility", "k_surface_resolve", "k_surface_composite",
                                        "k_surface_begin", "k_surface_visibility_masked", "k_surface_resolve", "k_surface_composite", "k_surface_store_depth"]), names
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), scene.raw.cpu().numpy().view(np.uint32))
        untouched = ~(opaque_cov | masked_cov)
        np.testing.assert_array_equal(main.cpu().numpy()[untouched].view(np.uint32), scene.sky.cpu().numpy()[untouched].view(np.uint32))
    finally:
        rt.close()


def test_the_masked_pass_writes_the_depth_it_owns(ctx, scene):
    """begun from the OPAQUE prepass alone, the Masked node's pass leaves the masked prepass depth in the attachment"""
    rt = scene.runtime(["RenderScene:Masked"], tagged=True)
    try:
        main, depth = scene.sky.clone(), scene.opaque.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)
        assert status == 0 and [n for n in names if n.startswith("k_surface_vis")] == ["k_surface_visibility_masked"], (status, names)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), scene.raw.cpu().numpy().view(np.uint32))
    finally:
        rt.close()


def test_without_tags_the_frame_is_the_untagged_draws_through_the_plain_entry_point(ctx, scene):
    want, want_depth, _ = scene.through_the_c_abi(ctx, [[(0, False, True), (1, False, True), (2, False, True)]])
    rt = scene.runtime(["RenderScene"], tagged=False)
    try:
        main, depth = scene.sky.clone(), scene.raw.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)
        assert status == 0, status
        assert surface_launches(names, ["k_surface_begin"] + ["k_surface_visibility"] * 3 + ["k_surface_resolve", "k_surface_composite"]), names
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), scene.raw.cpu().numpy().view(np.uint32))   # no cutout draw: no depth write
    finally:
        rt.close()


def test_set_scene_tags_refuses_what_does_not_parse(ctx, scene):
    rt = scene.runtime(["RenderScene"], tagged=False)
    try:
        flags = (C.c_uint32 * 3)(0, 0, 3)
        for tags, f, n in ((b"Opaque,Masked", flags, 3), (b"Opaque,Masked,,", flags, 3), (b"Opaque,Ma sked,x", flags, 3), (b"a,b,c", (C.c_uint32 * 3)(0, 4, 0), 3),
                           (b"a,b", flags, 2), (b"a,b,c", None, 3)):
            assert rt.rt.sailor_rt_set_scene_tags(rt.h, tags, f, n) == -1, tags
        assert rt.rt.sailor_rt_set_scene_tags(rt.h, b"Opaque,,Masked", flags, 3) == 0
        assert rt.rt.sailor_rt_set_scene_tags(rt.h, None, (C.c_uint32 * 3)(0, 0, 0), 3) == 0
    finally:
        rt.close()
