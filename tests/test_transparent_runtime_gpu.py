"""The Transparent render queue through the C++ host mirror: a `.renderer` text with the shipped frame's two RenderScene nodes' kind plus one with `Tag: Transparent`,
over tests/test_gltf_runtime_gpu.py's scene -- the glTF ground Opaque, the Standard boxes (Additive) and the glTF cutout quad (AlphaBlending) tagged Transparent
with z-write off through sailor_rt_set_scene_tags / _set_scene_blend.  The executed regions name the pass, `Main` equals the Python route
(SurfacePass.transparent with the budget's layers) bit for bit, the depth attachment is untouched, the overflow is readable after the frame; a pass that mixes
z-write on and off, a Multiply batch, an indirect transparent pass and a split frame return the unsupported status; a frame without transparent batches is
today's."""
import ctypes as C

import numpy as np
import pytest
import torch

from sailor_amd import _lib
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, SurfacePass, linearize_depth
from sailor_amd.runtime_binding import Runtime
from test_gltf_runtime_gpu import MIXED, Scene
from test_masked_runtime_gpu import frame_launches, surface_launches

pytestmark = pytest.mark.gpu
UNSUPPORTED = -7
NONE, ADDITIVE, ALPHA, MULTIPLY = 0, 1, 2, 3


def renderer(transparent=True, culling=False):
    c = "  - GPUCulling: true\n" if culling else ""
    text = """---
frame:
- name: LightCulling

- name: RenderScene
  string:
  - Tag: Opaque
  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer
"""
    if transparent:
        text += f"""
- name: RenderScene
  string:
  - Tag: Transparent
{c}  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer
"""
    return text


class TransparentScene(Scene):
    """the depth attachment is the ground's alone (what the prepass and the opaque pass of this frame leave); the boxes and the quad are the Transparent queue's"""

    def __init__(self, ctx):
        super().__init__(ctx)
        frame = self.f.cam.frame
        vertices = self.vertices.cpu().numpy()
        positions = torch.from_numpy(np.ascontiguousarray(vertices[:, 2:5])).to(ctx.device)
        inst = self.instances.cpu().numpy().view(np.uint8).reshape(-1, 96)
        model_only = torch.from_numpy(np.ascontiguousarray(inst[:, :64]).view(np.float32)).to(ctx.device)
        self.depth = torch.zeros((self.H, self.W), dtype=torch.float32, device=ctx.device)
        count, n, fi, vo, fin = self.batches[1].tolist()
        _lib.check(ctx._lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(frame), positions.data_ptr() + 12 * vo, self.indices.data_ptr() + 4 * fi, count // 3,
                                                           model_only.data_ptr() + 64 * fin, None, n, self.W, self.H, self.depth.data_ptr(), _lib.RASTER_CULL_BACK, None),
                   "sailor_hip_raster_depth_camera", ctx.handle)
        self.lin = linearize_depth(ctx, frame, self.depth)
        self.tags = ["Transparent", "Opaque", "Transparent"]
        self.blend, self.z_write = [ADDITIVE, NONE, ALPHA], [0, 1, 0]
        ctx.synchronize()

    def draw_args(self, k, cull_back, cutout, gltf, blend):
        count, drawn, first_index, vertex_offset, first_instance = self.batches[k].tolist()
        return dict(vertices=self.vertices[vertex_offset:], indices=self.indices[first_index:first_index + count], instance_ids=None, num_drawn=drawn,
                    first_instance=first_instance, cull_back=cull_back, alpha_cutout=cutout, gltf=gltf, blend=blend)

    def python_route(self, ctx, layers, transparent=True):
        """the Opaque node's pass as the backend runs it, then SurfacePass.transparent -> (Main, the counters)"""
        frame, n = self.f.cam.frame, len(self.f.lights)
        fp = ForwardPlus(ctx, self.W, self.H, n, prepared=PreparedLights(ctx, self.lights, n))
        fp.cull(frame, self.lights, n, self.lin)
        main = self.sky.clone()
        sp = SurfacePass(ctx, self.W, self.H)
        sp.begin(self.depth)
        self.draw(sp, 1, gltf=True, cutout=False, cull_back=True)
        surface, _, _, _, emissive = sp.resolve_gltf(frame, self.instances, self.materials, self.textures, self.num_textures)
        sp.composite_gltf(fp.shade(frame, surface, self.lights, n), emissive, main)
        counts = None
        if transparent:
            draws = [self.draw_args(0, True, False, False, "additive"), self.draw_args(2, False, True, True, "alpha")]
            counts = sp.transparent(frame, draws, self.instances, self.materials, self.textures, self.num_textures, self.depth,
                                    lambda surface, ao: fp.shade(frame, surface, self.lights, n), main, layers=layers).cpu().numpy()
        ctx.synchronize()
        return main.cpu().numpy(), counts

    def runtime_from(self, text, main, depth, blend=None, z_write=None, tags=None):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.set_camera(self.f.cam)
        loaded = rt.load_renderer(text)
        assert loaded[1] == 0, loaded
        rt.set_color_target("Main", main)
        rt.set_render_target("DepthBuffer", depth)
        rt.set_lights(self.f.lights)
        rt.set_depth(self.lin)
        rt.set_scene(self.vertices, self.indices, self.instances, self.materials, self.textures, self.num_textures, self.batches)
        rt.set_scene_tags(self.tags if tags is None else tags, self.flags)
        rt.set_scene_shaders(self.shaders)
        rt.set_scene_blend(self.blend if blend is None else blend, self.z_write if z_write is None else z_write)
        return rt


@pytest.fixture(scope="module")
def scene(ctx):
    return TransparentScene(ctx)


@pytest.mark.parametrize("layers", [4, 1])
def test_main_equals_the_python_route_and_the_overflow_is_readable(ctx, scene, layers):
    want, counts = scene.python_route(ctx, layers)
    assert counts[0] > 1000 and counts[1] > 100, counts     # more than one layer: boxes over boxes, boxes over the quad
    opaque_only, _ = scene.python_route(ctx, layers, transparent=False)
    assert (want.view(np.uint32) != opaque_only.view(np.uint32)).any(axis=-1).sum() > 1000
    main, depth = scene.sky.clone(), scene.depth.clone()
    rt = scene.runtime_from(renderer(), main, depth)
    try:
        if layers != 4:
            rt.set_transparent_layers(layers)      # (4 is the default)
        assert rt.transparent_overflow() == 0      # no pass recorded yet
        status, names = frame_launches(rt)
        assert status == 0, status
        assert "RenderScene QueueTag:Transparent" in rt.last_frame_regions() and "RenderScene QueueTag:Opaque" in rt.last_frame_regions(), rt.last_frame_regions()
        per_layer = ["k_surface_begin", "k_surface_peel", "k_surface_peel_gltf", "k_surface_peel_commit", "k_surface_resolve_gltf", "k_surface_blend"]
        opaque = ["k_surface_begin", "k_surface_visibility_gltf", "k_surface_resolve_gltf", "k_surface_composite_gltf"]   # the Opaque node's pass before it
        assert surface_launches(names, opaque + per_layer * layers + per_layer[:4]), names
        torch.cuda.synchronize()
        np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), scene.depth.cpu().numpy().view(np.uint32))   # the attachment is read only
        assert rt.transparent_overflow() == int(counts[layers])
        assert counts[layers] > 0 and (layers == 4 or counts[1] > 1000), counts   # the boxes stack deeper than either budget: both frames overflow
    finally:
        rt.close()


def test_every_refusal_returns_its_status(ctx, scene):
    def status_of(text=None, **how):
        main, depth = scene.sky.clone(), scene.depth.clone()
        rt = scene.runtime_from(text or renderer(), main, depth, **how)
        try:
            return frame_launches(rt)[0], main
        finally:
            rt.close()
    # z-write on and off in one pass: the quad keeps its tag and its blend but writes depth
    assert status_of(z_write=[0, 1, 1])[0] == UNSUPPORTED
    assert status_of(z_write=[1, 1, 0])[0] == UNSUPPORTED
    # a Multiply batch: nothing of the pass is launched, Main is the opaque pass's
    status, main = status_of(blend=[MULTIPLY, NONE, ALPHA])
    assert status == UNSUPPORTED
    torch.cuda.synchronize()
    np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), scene.python_route(ctx, 4, transparent=False)[0].view(np.uint32))
    # an indirect transparent pass
    assert status_of(renderer(culling=True))[0] == UNSUPPORTED
    # a split frame
    main, depth = scene.sky.clone(), scene.depth.clone()
    rt = scene.runtime_from(renderer(), main, depth)
    try:
        rt.set_frame_split(0, 2)
        assert frame_launches(rt)[0] == UNSUPPORTED
    finally:
        rt.close()
    # set_scene_blend refuses a wrong count and an unknown mode, and changes nothing then
    rt = scene.runtime_from(renderer(), scene.sky.clone(), scene.depth.clone())
    try:
        for bad in (([ADDITIVE, NONE], [0, 1]), ([ADDITIVE, NONE, 4], [0, 1, 0]), ([ADDITIVE, NONE, ALPHA], [0, 1, 2])):
            with pytest.raises(Exception):
                rt.set_scene_blend(*bad)
        for bad in (0, 65, -1):
            with pytest.raises(Exception):
                rt.set_transparent_layers(bad)
        assert frame_launches(rt)[0] == 0
    finally:
        rt.close()


def test_a_frame_without_transparent_batches_is_todays(ctx, scene):
    """every batch z-writing and blend None, through build_graph's one RenderScene node: test_gltf_runtime_gpu's frame and launches, bit for bit, with and
    without the call"""
    want, want_depth, cov, _ = scene.through_the_c_abi(ctx, MIXED)
    for call in (False, True):
        rt = scene.runtime(scene.shaders)
        try:
            if call:
                rt.set_scene_blend([NONE] * 3, [1] * 3)
            main, depth = scene.sky.clone(), scene.raw.clone()
            rt.set_scene_targets(main, depth)
            status, names = frame_launches(rt)
            assert status == 0, status
            assert surface_launches(names, ["k_surface_begin", "k_surface_visibility", "k_surface_visibility_gltf", "k_surface_visibility_gltf", "k_surface_resolve_gltf",
                                            "k_surface_composite_gltf", "k_surface_store_depth"]), names
            torch.cuda.synchronize()
            np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
            np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
            assert rt.transparent_overflow() == 0
        finally:
            rt.close()
