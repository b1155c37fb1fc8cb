"""Mip-mapped material textures through the C++ host mirror: tests/test_gltf_runtime_gpu.py's mixed scene (Standard boxes, a glTF ground, a glTF cutout quad)
over texture tables with full chains.  With Runtime.set_scene(..., texture_levels=...) one RenderScene node records the `_lod` entry points and `Main` and the
depth attachment equal the C-ABI `_lod` sequence bit for bit; without texture_levels the same tables give the frame and the launches of before; and
HipGraphicsDriver::GenerateMipMaps on a 2-D RGBA8 texture leaves the C-ABI's chain."""
import numpy as np
import pytest
import torch

import gltf_cases
import lod_cases
import lod_ref
import masked_cases
from sailor_amd import host
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, SurfacePass, linearize_depth, upload_textures
from sailor_amd.runtime_binding import Runtime
from test_gltf_runtime_gpu import MIXED, Scene
from test_masked_runtime_gpu import frame_launches, surface_launches
from test_surface_runtime_gpu import build

pytestmark = pytest.mark.gpu


class LodScene(Scene):
    """the mixed scene with every texture's chain generated on the device and the Masked prepass drawn at the implicit level of detail"""

    def __init__(self, ctx):
        super().__init__(ctx)
        _, _, _, _, _, textures, srgb, _ = build()
        self.images, self.srgb = textures + [masked_cases.checker(4), gltf_cases.rgb_texture(4, 4, 9)], srgb + [True, True]
        self.textures, self.num_textures, self.keep = upload_textures(ctx, self.images, self.srgb, mips=True)
        self.levels = [host.texture_mip_levels(i.shape[1], i.shape[0]) for i in self.images]
        self.flat_raw = self.raw                      # the prepass of the one-level route, as the parent class drew it
        self.raw = self.opaque.clone()
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(self.raw)
        self.draw(sp, 2, gltf=True, cutout=True, cull_back=False, lod=True)
        sp.store_depth(self.raw)
        self.lod_linear = linearize_depth(ctx, self.f.cam.frame, self.raw)
        ctx.synchronize()

    def draw(self, sp, k, gltf, cutout, cull_back, lod=False):
        count, drawn, first_index, vertex_offset, first_instance = self.batches[k].tolist()
        tables = dict(materials=self.materials, textures=self.textures, num_textures=self.num_textures) if cutout or gltf or lod else {}
        sp.draw(self.f.cam.frame, vertices=self.vertices[vertex_offset:], indices=self.indices[first_index:first_index + count], instances=self.instances, instance_ids=None,
                num_drawn=drawn, first_instance=first_instance, cull_back=cull_back, alpha_cutout=cutout, gltf=gltf, lod=lod, **tables)

    def through_the_c_abi_lod(self, ctx, draws):
        """one RenderScene pass over mip-mapped tables as the backend runs it -> (Main, the depth attachment after it, coverage)"""
        frame, n = self.f.cam.frame, len(self.f.lights)
        fp = ForwardPlus(ctx, self.W, self.H, n, prepared=PreparedLights(ctx, self.lights, n))
        fp.cull(frame, self.lights, n, self.lod_linear)
        main, depth = self.sky.clone(), self.raw.clone()
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(depth)
        for k, gltf, cutout, cull_back in draws:
            self.draw(sp, k, gltf, cutout, cull_back, lod=True)
        surface, _, cov, ao_out, emissive = sp.resolve_lod(frame, self.instances, self.materials, self.textures, self.num_textures)
        sp.composite_gltf(fp.shade(frame, surface, self.lights, n), emissive, main)
        sp.store_depth(depth)
        ctx.synchronize()
        return main.cpu().numpy(), depth.cpu().numpy(), cov.cpu().numpy().astype(bool)

    def runtime(self, shaders, texture_levels=None, linear=None):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.build_graph(["LightCulling", "RenderScene"])
        rt.set_camera(self.f.cam)
        rt.set_lights(self.f.lights)
        rt.set_depth(self.linear if linear is None else linear)
        rt.set_scene(self.vertices, self.indices, self.instances, self.materials, self.textures, self.num_textures, self.batches, texture_levels=texture_levels)
        rt.set_scene_tags(["", "", ""], self.flags)
        rt.set_scene_shaders(shaders)
        return rt


@pytest.fixture(scope="module")
def scene(ctx):
    return LodScene(ctx)


def test_with_texture_levels_the_frame_is_the_c_abi_lod_sequence(ctx, scene):
    want, want_depth, cov = scene.through_the_c_abi_lod(ctx, MIXED)
    assert cov.mean() > 0.3 and max(scene.levels) == 5
    rt = scene.runtime(scene.shaders, texture_levels=scene.levels, linear=scene.lod_linear)
    try:
        main, depth = scene.sky.clone(), scene.raw.clone()
        rt.set_scene_targets(main, depth)
        status, names = frame_launches(rt)
        assert status == 0, status
        assert surface_launches(names, ["k_surface_begin", "k_surface_visibility_lod", "k_surface_visibility_lod_gltf", "k_surface_visibility_lod_gltf", "k_surface_resolve_lod",
                                        "k_surface_composite_gltf", "k_surface_store_depth"]), names
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
        np.testing.assert_array_equal(main.cpu().numpy()[~cov].view(np.uint32), scene.sky.cpu().numpy()[~cov].view(np.uint32))
    finally:
        rt.close()
    # the chains reach the picture: the one-level sequence over the same tables gives another frame
    flat = scene.through_the_c_abi(ctx, MIXED)[0]
    assert (flat.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum() > 100


def test_without_texture_levels_the_frame_and_the_launches_are_todays(ctx, scene):
    raw, scene.raw = scene.raw, scene.flat_raw        # the one-level route's own prepass
    try:
        want, want_depth, cov, _ = scene.through_the_c_abi(ctx, MIXED)
        for levels in (None, [1] * scene.num_textures, [0] * scene.num_textures):
            rt = scene.runtime(scene.shaders, texture_levels=levels)
            try:
                main, depth = scene.sky.clone(), scene.raw.clone()
                rt.set_scene_targets(main, depth)
                status, names = frame_launches(rt)
                assert status == 0, status
                assert surface_launches(names, ["k_surface_begin", "k_surface_visibility", "k_surface_visibility_gltf", "k_surface_visibility_gltf", "k_surface_resolve_gltf",
                                                "k_surface_composite_gltf", "k_surface_store_depth"]), names
                torch.cuda.synchronize()
                np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
                np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
            finally:
                rt.close()
    finally:
        scene.raw = raw


def test_texture_levels_of_another_length_are_refused(ctx, scene):
    rt = scene.runtime(scene.shaders)
    try:
        with pytest.raises(Exception):
            rt.set_scene(scene.vertices, scene.indices, scene.instances, scene.materials, scene.textures, scene.num_textures, scene.batches,
                         texture_levels=[2] * (scene.num_textures + 1))
    finally:
        rt.close()


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_generate_mip_maps_on_a_2d_texture_leaves_the_c_abi_chain(ctx, srgb):
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        for k, (w, h) in enumerate(lod_cases.EXTENTS):
            img = lod_cases.random_texture(w, h, 70 + k)
            got = rt.generate_texture_mips(img, srgb)
            _, _, keep = upload_textures(ctx, [img], [srgb], mips=True)
            ctx.synchronize()
            np.testing.assert_array_equal(got, keep[0].cpu().numpy().view(np.uint32), err_msg=f"{w} x {h}")
            np.testing.assert_array_equal(got, lod_ref.flat_chain(lod_ref.build_chain(img, srgb)), err_msg=f"{w} x {h} against the restatement")
    finally:
        rt.close()
