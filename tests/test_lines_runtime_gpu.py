"""The DebugDraw node through the C++ host mirror: a `.renderer` text with LightCulling, a RenderScene without Clear and DebugDraw, as DefaultRenderer.renderer
orders them, over test_masked_runtime_gpu's scene.  Lines are submitted through the binding (Runtime.debug_draw_*), ticked (Runtime.debug_tick) and drawn by the
node: `Main` and `DepthBuffer` equal the C-ABI sequence bit for bit; a line whose lifetime is shorter than the tick is drawn in the frame of the tick that expires
it and not in the next; a frame with no lines launches nothing from debug_lines.hip."""
import numpy as np
import pytest
import torch

from sailor_amd import _lib, host
from sailor_amd.forward_plus import DebugLinesPass, ForwardPlus, PreparedLights
from sailor_amd.runtime_binding import Runtime, load
from test_masked_runtime_gpu import Scene

pytestmark = pytest.mark.gpu

RENDERER = """---
frame:
- name: LightCulling

- name: RenderScene
  string:
  - Tag: Opaque
  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer

- name: DebugDraw
  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer
"""
PASS = [(0, False, True), (1, False, True), (2, False, True)]   # the scene's three batches, untagged: all through the plain draw, back faces culled


@pytest.fixture(scope="module")
def scene(ctx):
    return Scene(ctx)


def runtime(scene):
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    rt.set_camera(scene.f.cam)
    assert rt.load_renderer(RENDERER) == (3, 0, 0)   # DebugDraw has a node class: created, not skipped
    rt.set_lights(scene.f.lights)
    rt.set_depth(scene.linear)
    rt.set_scene(scene.vertices, scene.indices, scene.instances, scene.materials, scene.textures, scene.num_textures, scene.batches)
    return rt


def targets(rt, scene):
    main, depth = scene.sky.clone(), scene.raw.clone()
    rt.set_scene_targets(main, depth)          # RenderScene's attachments
    rt.set_color_target("Main", main)          # ... and the same images under the names DebugDraw's entry gives
    rt.set_render_target("DepthBuffer", depth)
    return main, depth


def frame_launches(rt):
    before, _ = rt.launch_log(0)
    status = rt.process_frame()
    rt.wait_idle()
    after, names = rt.launch_log(16)
    n = min(after - before, 16)
    return status, names[len(names) - n:] if n else []


def through_the_c_abi(ctx, scene, line_vertices):
    """RenderScene's pass, then the DebugDraw pass over `line_vertices` (VertexP3C4 records) -> (Main, DepthBuffer, pixels the lines own)"""
    n = len(scene.f.lights)
    fp = ForwardPlus(ctx, scene.W, scene.H, n, prepared=PreparedLights(ctx, scene.lights, n))
    fp.cull(scene.f.cam.frame, scene.lights, n, scene.linear)
    main, depth = scene.sky.clone(), scene.raw.clone()
    scene.one_pass(ctx, fp, main, depth, PASS)
    owned = 0
    if len(line_vertices):
        frame = scene.f.cam.frame
        vp = host.mat4_mul(np.float32(list(frame.projection)), np.float32(list(frame.view)))   # DrawDebugMesh(projection * view)
        dp = DebugLinesPass(ctx, scene.W, scene.H)
        dp.begin(depth)
        dp.draw(vp, torch.from_numpy(line_vertices.view(np.uint8).copy()).to(ctx.device))
        dp.resolve(main, depth)
        owned = int((dp.download_keys().astype(np.uint32) != 0).sum())
    ctx.synchronize()
    return main.cpu().numpy(), depth.cpu().numpy(), owned


def same(got, want):
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def submit_shapes(rt, scene):
    """an AABB round the scene's quad, the origin's axes, a sphere, the frustum of a narrower camera, an arrow: all with the default lifetime 0 (one frame)"""
    cam = scene.f.cam
    rt.debug_draw_aabb([-160, -5, -215], [160, 310, -185], (1, 1, 0, 1))
    rt.debug_draw_origin([0, 150, -200], np.eye(4, dtype=np.float32), 120.0)
    rt.debug_draw_sphere([0, 150, -200], 90.0, (0, 1, 1, 0.5))
    _, corners = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov * 0.5, cam.z_near * 2, min(cam.z_far, 600.0))
    rt.debug_draw_frustum(corners, (1, 0, 1, 1))
    rt.debug_draw_arrow([-100, 20, -150], [120, 200, -260], (0.2, 0.9, 0.3, 1))


def test_the_node_is_registered_and_the_shipped_entry_creates_it():
    assert load().sailor_rt_node_registered(b"DebugDraw") == 1   # FrameGraph/DebugDrawNode.cpp:16


def test_main_and_depth_equal_the_c_abi_sequence_and_lifetimes_end_after_their_frame(ctx, scene):
    rt = runtime(scene)
    try:
        submit_shapes(rt, scene)
        rt.debug_draw_line([-150, 10, -120], [150, 290, -280], (1, 0.5, 0, 1), duration=0.05)   # shorter than the tick
        rt.debug_draw_line([150, 10, -120], [-150, 290, -280], (0, 0.5, 1, 1), duration=10.0)   # stays
        first = rt.debug_vertices()
        lines = 12 + 3 + 176 + 12 + 4 + 2
        assert len(first) == 2 * lines
        assert first[:30].tobytes() == np.concatenate([                                         # the mirror and the host helpers build the same list
            host.debug_aabb([-160, -5, -215], [160, 310, -185], (1, 1, 0, 1)), host.debug_origin([0, 150, -200], np.eye(4), 120.0)]).tobytes()
        want, want_depth, owned = through_the_c_abi(ctx, scene, first)
        assert owned > 300, owned
        assert rt.debug_tick(0.1) == 2 * lines          # set before the lifetimes run down: everything is drawn in this tick's frame ...
        assert len(rt.debug_vertices()) == 2            # ... and only the long line is left afterwards
        main, depth = targets(rt, scene)
        status, names = frame_launches(rt)
        assert status == 0 and names[-3:] == ["k_surface_begin", "k_debug_lines_draw", "k_debug_lines_resolve"], (status, names)
        same(main, want)
        same(depth, want_depth)
        assert (want_depth != scene.raw.cpu().numpy()).sum() > 100    # the lines wrote depth

        second = rt.debug_vertices()
        np.testing.assert_array_equal(second["position"], np.float32([[150, 10, -120], [-150, 290, -280]]))
        want2, want_depth2, owned2 = through_the_c_abi(ctx, scene, second)
        assert 10 < owned2 < owned
        assert rt.debug_tick(0.1) == 2
        main, depth = targets(rt, scene)
        status, names = frame_launches(rt)
        assert status == 0 and names[-2:] == ["k_debug_lines_draw", "k_debug_lines_resolve"], (status, names)
        same(main, want2)                               # the short line is not drawn again
        same(depth, want_depth2)
        assert not np.array_equal(want2, want)
    finally:
        rt.close()


def test_a_frame_with_no_lines_launches_nothing_from_debug_lines(ctx, scene):
    want, want_depth, _ = through_the_c_abi(ctx, scene, np.zeros(0, _lib.VERTEX_P3C4_DTYPE))
    rt = runtime(scene)
    try:
        assert rt.debug_tick(0.1) == 0
        main, depth = targets(rt, scene)
        status, names = frame_launches(rt)
        assert status == 0 and names, (status, names)
        assert not [n for n in names if n.startswith("k_debug_lines")] and names.count("k_surface_begin") == 1, names   # DrawDebugMesh returned early
        same(main, want)
        same(depth, want_depth)
    finally:
        rt.close()
