"""glTF materials through the C++ host mirror: one RenderScene node over a scene whose batches mix Standard.shader (the boxes), Standard_glTF.shader (the ground)
and Standard_glTF.shader with ALPHA_CUTOUT (a double-sided checker-alpha quad), set through Runtime.set_scene_shaders.  `Main` and the depth attachment equal the
C-ABI sequence bit for bit; with no glTF batch the frame records the launches of before; set_scene_shaders refuses what it does not know and changes nothing then."""
import ctypes as C

import numpy as np
import pytest
import torch

import gltf_cases
import masked_cases
import surface_cases as cases
from sailor_amd import _lib, host
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, SurfacePass, linearize_depth, upload_lights, upload_textures
from sailor_amd.runtime_binding import Runtime
from test_masked_runtime_gpu import BATCH_ALPHA_CUTOUT, BATCH_DOUBLE_SIDED, frame_launches, surface_launches
from test_surface_runtime_gpu import build

pytestmark = pytest.mark.gpu
SHADER_STANDARD, SHADER_STANDARD_GLTF = 0, 1


class Scene:
    """test_surface_runtime_gpu's pool (boxes and a ground) plus a quad with a 4 x 4 alpha checker: three batches, the last two with glTF records in their slots"""

    def __init__(self, ctx):
        self.f, vertices, indices, inst, mats, textures, srgb, batches = build()
        dev = ctx.device
        self.W, self.H = self.f.cam.width, self.f.cam.height
        qv, qt = cases.quad(-1, -1, 1, 1, z=0.0, uv=((0, 0), (3, 0), (3, 3), (0, 3)))
        first_vertex, first_index, first_instance = len(vertices), len(indices), len(inst)
        vertices = np.concatenate([vertices, np.asarray(qv, np.float32)])
        indices = np.concatenate([indices, np.asarray(qt, np.uint32).reshape(-1)]).astype(np.uint32)
        models = list(inst["model"]) + [host.transform_matrix([0.0, 150.0, -200.0, 1.0], [0.0, 0.0, 0.0, 1.0], [150.0, 150.0, 150.0, 1.0])]
        slots = list(inst["materialInstance"])
        slots[-1] = 3                                          # the ground (the last instance of the pool): the glTF record of slot 3
        inst = cases.instances(models, slots + [2])            # the quad: the glTF record of slot 2
        textures, srgb = textures + [masked_cases.checker(4), gltf_cases.rgb_texture(4, 4, 9)], srgb + [True, True]
        mats = np.concatenate([mats, gltf_cases.gltf_material(base=(0.8, 0.9, 0.3, 1), emissive=(0.5, 0.1, 0.0, 0), metallic=0.1, roughness=0.7, cutoff=0.4,
                                                              samplers=(3, 1, 4, 4, 4)),
                               gltf_cases.gltf_material(base=(0.5, 0.7, 0.4, 1), emissive=(0.0, 0.05, 0.1, 0), metallic=0.2, roughness=0.9, normal_scale=0.5,
                                                        samplers=(0, 1, 4, 4, 2))])
        self.batches = np.concatenate([batches, np.uint32([[6, 1, first_index, first_vertex, first_instance]])])
        self.flags = [0, 0, BATCH_ALPHA_CUTOUT | BATCH_DOUBLE_SIDED]
        self.shaders = [SHADER_STANDARD, SHADER_STANDARD_GLTF, SHADER_STANDARD_GLTF]
        self.vertices, self.indices = torch.from_numpy(vertices).to(dev), torch.from_numpy(indices.view(np.int32)).to(dev)
        self.instances, self.materials = torch.from_numpy(inst.view(np.uint8).copy()).to(dev), torch.from_numpy(mats.view(np.uint8).copy()).to(dev)
        self.textures, self.num_textures, self.keep = upload_textures(ctx, textures, srgb)
        self.lights = upload_lights(self.f.lights, dev)
        frame = self.f.cam.frame
        # DepthPrepass `Tag: Opaque` (DepthOnly.shader, back faces culled) over the boxes and the ground, then the glTF cutout quad: begin, the draw, store_depth
        self.opaque = torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)
        positions = torch.from_numpy(np.ascontiguousarray(vertices[:, 2:5])).to(dev)
        model_only = torch.from_numpy(np.ascontiguousarray(inst["model"])).to(dev)
        for count, n, fi, vo, fin in self.batches[:2].tolist():
            _lib.check(ctx._lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(frame), positions.data_ptr() + 12 * vo, self.indices.data_ptr() + 4 * fi, count // 3,
                                                               model_only.data_ptr() + 64 * fin, None, n, self.W, self.H, self.opaque.data_ptr(), _lib.RASTER_CULL_BACK, None),
                       "sailor_hip_raster_depth_camera", ctx.handle)
        self.raw = self.opaque.clone()
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(self.raw)
        self.draw(sp, 2, gltf=True, cutout=True, cull_back=False)
        sp.store_depth(self.raw)
        self.linear = linearize_depth(ctx, frame, self.raw)
        self.sky = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (self.H, self.W, 4)).astype(np.float32)).to(dev)
        ctx.synchronize()

    def draw(self, sp, k, gltf, cutout, cull_back):
        count, drawn, first_index, vertex_offset, first_instance = self.batches[k].tolist()
        tables = dict(materials=self.materials, textures=self.textures, num_textures=self.num_textures) if cutout or gltf else {}
        sp.draw(self.f.cam.frame, vertices=self.vertices[vertex_offset:], indices=self.indices[first_index:first_index + count], instances=self.instances, instance_ids=None,
                num_drawn=drawn, first_instance=first_instance, cull_back=cull_back, alpha_cutout=cutout, gltf=gltf, **tables)

    def through_the_c_abi(self, ctx, draws):
        """one RenderScene pass as the backend runs it -> (Main, the depth attachment after it, coverage, the pixels glTF draws own)"""
        frame, n = self.f.cam.frame, len(self.f.lights)
        fp = ForwardPlus(ctx, self.W, self.H, n, prepared=PreparedLights(ctx, self.lights, n))
        fp.cull(frame, self.lights, n, self.linear)
        main, depth = self.sky.clone(), self.raw.clone()
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(depth)
        for k, gltf, cutout, cull_back in draws:
            self.draw(sp, k, gltf, cutout, cull_back)
        if any(g for _, g, _, _ in draws):
            surface, _, cov, ao_out, emissive = sp.resolve_gltf(frame, self.instances, self.materials, self.textures, self.num_textures)   # (no g_aoSampler is bound)
            sp.composite_gltf(fp.shade(frame, surface, self.lights, n), emissive, main)
            lit = emissive[..., :3].sum(-1) > 0
        else:
            surface, _, cov = sp.resolve(frame, self.instances, self.materials, self.textures, self.num_textures)
            sp.composite(fp.shade(frame, surface, self.lights, n), main)
            lit = torch.zeros_like(cov, dtype=torch.bool)
        if any(c for _, _, c, _ in draws):
            sp.store_depth(depth)
        ctx.synchronize()
        return main.cpu().numpy(), depth.cpu().numpy(), cov.cpu().numpy().astype(bool), lit.cpu().numpy()

    def runtime(self, shaders):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.build_graph(["LightCulling", "RenderScene"])
        rt.set_camera(self.f.cam)
        rt.set_lights(self.f.lights)
        rt.set_depth(self.linear)
        rt.set_scene(self.vertices, self.indices, self.instances, self.materials, self.textures, self.num_textures, self.batches)
        rt.set_scene_tags(["", "", ""], self.flags)
        if shaders is not None:
            rt.set_scene_shaders(shaders)
        return rt


@pytest.fixture(scope="module")
def scene(ctx):
    return Scene(ctx)


MIXED = [(0, False, False, True), (1, True, False, True), (2, True, True, False)]
STANDARD_LAUNCHES = ["k_surface_begin", "k_surface_visibility", "k_surface_visibility", "k_surface_visibility_masked", "k_surface_resolve", "k_surface_composite",
                     "k_surface_store_depth"]


def test_main_and_depth_of_a_mixed_scene_equal_the_c_abi_sequence(ctx, scene):
    want, want_depth, cov, lit = scene.through_the_c_abi(ctx, MIXED)
    assert cov.mean() > 0.3 and lit.sum() > 300 and (cov & ~lit).sum() > 300   # glTF pixels with an emissive term, and Standard ones
    np.testing.assert_array_equal(want_depth.view(np.uint32), scene.raw.cpu().numpy().view(np.uint32))
    assert (scene.raw != scene.opaque).sum() > 100   # the cutout quad wrote depth
    rt = scene.runtime(scene.shaders)
    try:
        main, depth = scene.sky.clone(), scene.raw.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)
        assert status == 0, status
        assert surface_launches(names, ["k_surface_begin", "k_surface_visibility", "k_surface_visibility_gltf", "k_surface_visibility_gltf", "k_surface_resolve_gltf",
                                        "k_surface_composite_gltf", "k_surface_store_depth"]), names
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), scene.raw.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(main.cpu().numpy()[~cov].view(np.uint32), scene.sky.cpu().numpy()[~cov].view(np.uint32))
    finally:
        rt.close()


@pytest.mark.parametrize("shaders", [None, [SHADER_STANDARD] * 3], ids=["never set", "all Standard"])
def test_without_a_gltf_batch_the_frame_records_the_launches_of_before(ctx, scene, shaders):
    want, _, _, _ = scene.through_the_c_abi(ctx, [(0, False, False, True), (1, False, False, True), (2, False, True, False)])
    rt = scene.runtime(shaders)
    try:
        main, depth = scene.sky.clone(), scene.raw.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)
        assert status == 0, status
        assert surface_launches(names, STANDARD_LAUNCHES) and not [n for n in names if "gltf" in n], names
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
    finally:
        rt.close()


def test_set_scene_shaders_refuses_what_it_does_not_know_and_changes_nothing(ctx, scene):
    rt = scene.runtime(None)
    try:
        good = (C.c_uint32 * 3)(0, 1, 1)
        for shaders, n in (((C.c_uint32 * 3)(0, 2, 1), 3), ((C.c_uint32 * 3)(1, 1, 0xFFFFFFFF), 3), (good, 2), (good, 4), (good, -1), (None, 3)):
            assert rt.rt.sailor_rt_set_scene_shaders(rt.h, shaders, n) == -1, (None if shaders is None else list(shaders), n)
        main, depth = scene.sky.clone(), scene.raw.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)   # (1, 1, 0xFFFFFFFF) was refused as a whole: no batch became a glTF batch
        assert status == 0 and surface_launches(names, STANDARD_LAUNCHES), (status, names)
        assert rt.rt.sailor_rt_set_scene_shaders(rt.h, good, 3) == 0
        status, names = frame_launches(rt)
        assert status == 0 and [n for n in names if n.startswith("k_surface_vis")] == ["k_surface_visibility", "k_surface_visibility_gltf", "k_surface_visibility_gltf"], names
        assert rt.rt.sailor_rt_set_scene_shaders(rt.h, (C.c_uint32 * 3)(0, 0, 0), 3) == 0
        status, names = frame_launches(rt)
        assert status == 0 and surface_launches(names, STANDARD_LAUNCHES), (status, names)
    finally:
        rt.close()
