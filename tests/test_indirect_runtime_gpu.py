"""GPU-driven draws through the C++ host mirror: a `.renderer` text with `DepthPrepass` Opaque (ClearDepth, GPUCulling), `DepthPrepass` Masked, LightCulling,
then `RenderScene` Opaque and Masked with `GPUCulling: true`, over test_masked_runtime_gpu's scene plus a fourth batch of boxes most of which stand outside the
view.  `DepthBuffer` after the prepasses is the prepass depth of the C-ABI bit for bit (from an attachment that held garbage: ClearDepth), `Main` equals the same
frame graph without the `GPUCulling` strings and the C-ABI sequence, the culls are launched before the first draw and the draws are the indirect kernels, every
node's downloaded instanceCounts are the C oracle's, a second frame with the camera turned is that frame's (the nodes refill their records), and a shader
without a route under DrawIndexedIndirect is refused with SAILOR_HIP_ERR_UNSUPPORTED, which the next process_frame() returns because the driver's status is
sticky (the refusal is recorded by a helper in a submission of its own, not inside that frame)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import surface_cases as cases
from oracle import oracle
from sailor_amd import _lib, host
from sailor_amd.forward_plus import SurfacePass, linearize_depth, masked_depth_prepass
from sailor_amd.runtime_binding import Runtime
from test_masked_runtime_gpu import Scene as MaskedScene

pytestmark = pytest.mark.gpu
UNSUPPORTED = -7   # SAILOR_HIP_ERR_UNSUPPORTED


def renderer(culling: bool) -> str:
    c = "  - GPUCulling: true\n" if culling else ""
    return f"""---
frame:
- name: DepthPrepass
  string:
  - Tag: Opaque
  - ClearDepth: true
{c}  renderTargets:
  - depthStencil: DepthBuffer

- name: DepthPrepass
  string:
  - Tag: Masked
{c}  renderTargets:
  - depthStencil: DepthBuffer

- name: LightCulling

- name: RenderScene
  string:
  - Tag: Opaque
{c}  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer

- name: RenderScene
  string:
  - Tag: Masked
{c}  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer
"""


PREPASS_ONLY = """---
frame:
- name: DepthPrepass
  string:
  - Tag: Opaque
  - ClearDepth: true
  - GPUCulling: true
  renderTargets:
  - depthStencil: DepthBuffer

- name: DepthPrepass
  string:
  - Tag: Masked
  - GPUCulling: true
  renderTargets:
  - depthStencil: DepthBuffer
"""
NODE_BATCHES = {0: [0, 1, 3], 1: [2], 3: [0, 1, 3], 4: [2]}   # graph node -> the batches of its queue, in drawing order
EXTRA_INSIDE, EXTRA_OUTSIDE = 4, 8


class Scene(MaskedScene):
    """test_masked_runtime_gpu's three batches (boxes, ground: Opaque; the checker quad: Masked) with bounding spheres on every record, and a fourth, Opaque batch
    of twelve more boxes: four in the view, eight far outside it (to the left, to the right, behind the camera)"""

    def __init__(self, ctx):
        super().__init__(ctx)
        dev = ctx.device
        inst = self.instances.cpu().numpy().view(host.INSTANCE_DTYPE).copy()
        first = len(inst)
        rng = np.random.default_rng(33)
        inside = [[rng.uniform(-60, 60), rng.uniform(110, 190), rng.uniform(-260, -120)] for _ in range(EXTRA_INSIDE)]
        outside = [[(-6000.0, 150.0, -100.0), (6000.0, 150.0, -100.0), (0.0, 150.0, 900.0)][k % 3] for k in range(EXTRA_OUTSIDE)]
        order = [outside[0], inside[0], outside[1], outside[2], inside[1], inside[2], outside[3], outside[4], outside[5], inside[3], outside[6], outside[7]]
        models = [host.transform_matrix([*p, 1.0], (lambda q: q / np.linalg.norm(q))(rng.normal(size=4)), [*rng.uniform(8, 30, 3), 1.0]) for p in order]
        extra = cases.instances(models, rng.integers(0, 2, len(models)))
        inst = np.concatenate([inst.view(np.uint8).reshape(-1, 96), extra.view(np.uint8).reshape(-1, 96)]).reshape(-1).view(host.INSTANCE_DTYPE)
        # bounding spheres in model space: the unit cube's, the ground quad's, the checker quad's
        inst["sphereBounds"][:] = (0.0, 0.0, 0.0, np.sqrt(3.0))
        ground, quad = int(self.batches[1][4]), int(self.batches[2][4])
        inst["sphereBounds"][ground] = (0.0, 60.0, -400.0, 700.0)
        inst["sphereBounds"][quad] = (0.0, 0.0, 0.0, 1.5)
        box = self.batches[0]
        self.batches = np.concatenate([self.batches, np.uint32([[box[0], len(models), box[2], box[3], first]])])
        self.tags, self.flags = self.tags + ["Opaque"], self.flags + [0]
        self.host_instances = inst
        self.instances = torch.from_numpy(inst.view(np.uint8).copy()).to(dev)
        # the prepass depth again, with the fourth batch among the Opaque ones
        frame = self.f.cam.frame
        self.raw, self.opaque = self.prepass(ctx, frame)
        self.linear = linearize_depth(ctx, frame, self.raw)
        ctx.synchronize()

    def prepass(self, ctx, frame):
        """DepthPrepass Opaque (DepthOnly.shader, back faces culled) then Masked through the C-ABI, un-culled -> (raw depth, the Opaque depth alone)"""
        vertices = self.vertices.cpu().numpy()
        positions = torch.from_numpy(np.ascontiguousarray(vertices[:, 2:5])).to(ctx.device)
        model_only = torch.from_numpy(np.ascontiguousarray(self.host_instances["model"])).to(ctx.device)
        opaque = torch.zeros((self.H, self.W), dtype=torch.float32, device=ctx.device)
        for k in (0, 1, 3):
            count, n, fi, vo, fin = self.batches[k].tolist()
            _lib.check(ctx._lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(frame), positions.data_ptr() + 12 * vo, self.indices.data_ptr() + 4 * fi, count // 3,
                                                               model_only.data_ptr() + 64 * fin, None, n, self.W, self.H, opaque.data_ptr(), _lib.RASTER_CULL_BACK, None),
                       "sailor_hip_raster_depth_camera", ctx.handle)
        raw = masked_depth_prepass(SurfacePass(ctx, self.W, self.H), frame, opaque.clone(), [self.draw_args(2)], self.instances, self.materials, self.textures,
                                   self.num_textures)
        ctx.synchronize()
        return raw, opaque

    def runtime_from(self, text, main, depth, cam=None):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.set_camera(cam or self.f.cam)
        loaded = rt.load_renderer(text)
        assert loaded[1] == 0, loaded   # DepthPrepass has a node class: created, not skipped
        rt.set_color_target("Main", main)          # the per-frame targets the entries name
        rt.set_render_target("DepthBuffer", depth)
        rt.set_lights(self.f.lights)
        rt.set_depth(self.linear)
        rt.set_scene(self.vertices, self.indices, self.instances, self.materials, self.textures, self.num_textures, self.batches)
        rt.set_scene_tags(self.tags, self.flags)
        return rt

    def oracle_counts(self, frame, batches):
        """the C oracle's cull and compaction over a node's own records: its queue's batches packed in drawing order"""
        packed = np.concatenate([self.host_instances[int(self.batches[k][4]): int(self.batches[k][4]) + int(self.batches[k][1])].view(np.uint8).reshape(-1, 96)
                                 for k in batches]).reshape(-1).view(host.INSTANCE_DTYPE)
        commands, at = np.zeros((len(batches), 5), np.uint32), 0
        for j, k in enumerate(batches):
            commands[j] = (self.batches[k][0], self.batches[k][1], self.batches[k][2], self.batches[k][3], at)
            at += int(self.batches[k][1])
        _, after = oracle.mesh_cull_compact(frame, packed, len(packed), 0, commands)
        return commands, after


def garbage_depth(scene):
    return torch.full((scene.H, scene.W), 0.75, dtype=torch.float32, device=scene.raw.device)


def frame_launches(rt):
    before, _ = rt.launch_log(0)
    status = rt.process_frame()
    rt.wait_idle()
    after, names = rt.launch_log(16)
    n = min(after - before, 16)
    return status, names[len(names) - n:] if n else [], after - before


def same(got, want, what=""):
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32) if torch.is_tensor(want) else want.view(np.uint32), err_msg=what)


def check_counts(scene, rt, frame):
    total_culled = 0
    for node, batches in NODE_BATCHES.items():
        written, want = scene.oracle_counts(frame, batches)
        got = rt.node_indirect_commands(node)
        np.testing.assert_array_equal(got, want, err_msg=f"node {node}")
        np.testing.assert_array_equal(got[:, [0, 2, 3, 4]], written[:, [0, 2, 3, 4]], err_msg=f"node {node}: only instanceCount is rewritten")
        total_culled += int(written[:, 1].sum() - got[:, 1].sum())
    return total_culled


@pytest.fixture(scope="module")
def scene(ctx):
    return Scene(ctx)


def test_depth_main_counts_and_a_second_frame_with_the_camera_turned(ctx, scene):
    cam = scene.f.cam
    want_main, want_depth, (opaque_cov, masked_cov) = scene.through_the_c_abi(ctx, [[(0, False, True), (1, False, True), (3, False, True)], [(2, True, False)]])
    assert opaque_cov.mean() > 0.3 and masked_cov.sum() > 300
    # the second frame's camera: turned by 45 degrees -- other survivors, from refilled records
    turned = copy.copy(cam)
    turned.world = host.transform_matrix([0.0, 150.0, 0.0, 1.0], [0.0, np.sin(np.pi / 8), 0.0, np.cos(np.pi / 8)], [1.0, 1.0, 1.0, 1.0])
    turned.frame = host.fill_frame_data(turned.world, cam.fov, cam.z_near, cam.z_far, cam.width, cam.height)
    turned_raw, _ = scene.prepass(ctx, turned.frame)
    first_counts = [scene.oracle_counts(cam.frame, b)[1][:, 1].tolist() for b in NODE_BATCHES.values()]
    second_counts = [scene.oracle_counts(turned.frame, b)[1][:, 1].tolist() for b in NODE_BATCHES.values()]
    assert first_counts != second_counts
    runs = {}
    for culling in (True, False):   # (one runtime at a time: the renderer is the process's)
        main, depth = scene.sky.clone(), garbage_depth(scene)
        rt = scene.runtime_from(renderer(culling), main, depth)
        try:
            status, names, launched = frame_launches(rt)
            assert status == 0, (culling, status, names)
            torch.cuda.synchronize()
            same(depth, scene.raw, f"DepthBuffer after the prepasses, culling={culling}")
            runs[culling] = main.clone()
            own = [n for n in names if n.startswith("k_surface")]
            if culling:
                assert all(n.startswith("k_surface_visibility_indirect") for n in own if n.startswith("k_surface_visibility")), names
                assert own[-5:] == ["k_surface_begin", "k_surface_visibility_indirect", "k_surface_resolve", "k_surface_composite", "k_surface_store_depth"], names
                assert check_counts(scene, rt, cam.frame) >= 2 * EXTRA_OUTSIDE   # the far boxes are culled in each of the two Opaque nodes at least
            else:   # without the strings RenderScene records DrawIndexed as before
                assert own[-5:] == ["k_surface_begin", "k_surface_visibility_masked", "k_surface_resolve", "k_surface_composite", "k_surface_store_depth"], names
            main.copy_(scene.sky); depth.fill_(0.25)
            rt.set_camera(turned)
            assert rt.process_frame() == 0
            rt.wait_idle()
            same(depth, turned_raw, f"DepthBuffer of the turned frame, culling={culling}")
            runs[culling, "turned"] = main.clone()
            if culling:
                check_counts(scene, rt, turned.frame)
                main.copy_(scene.sky); depth.fill_(0.5)
                rt.set_camera(cam)
                assert rt.process_frame() == 0   # and back: the first frame again
                rt.wait_idle()
                same(depth, scene.raw)
                same(main, runs[True], "the first frame again")
        finally:
            rt.close()
    same(runs[True, "turned"], runs[False, "turned"], "Main of the turned frame with and without the GPUCulling strings")
    same(runs[True], runs[False], "Main with and without the GPUCulling strings")
    np.testing.assert_array_equal(runs[True].cpu().numpy().view(np.uint32), want_main.view(np.uint32))
    untouched = ~(opaque_cov | masked_cov)
    np.testing.assert_array_equal(runs[True].cpu().numpy()[untouched].view(np.uint32), scene.sky.cpu().numpy()[untouched].view(np.uint32))


def test_the_culls_are_launched_before_the_first_draw_and_the_draws_are_indirect(ctx, scene):
    main, depth = scene.sky.clone(), garbage_depth(scene)
    rt = scene.runtime_from(PREPASS_ONLY, main, depth)
    try:
        status, names, launched = frame_launches(rt)
        assert status == 0, (status, names)
        surface = [n for n in names if n.startswith("k_surface")]
        assert surface == ["k_surface_begin"] + ["k_surface_visibility_indirect"] * 3 + ["k_surface_store_depth", "k_surface_begin", "k_surface_visibility_indirect",
                                                                                       "k_surface_store_depth"], names
        # the mesh cull's kernels are launched outside the context's launch log (as they always were), so their place is read from the debug regions in the
        # order the driver EXECUTED their begin commands while it submitted the frame's lists, i.e. the order their work went onto the stream: both nodes'
        # "GPU Culling" dispatches, on the transfer list, come before the region of the first draw
        regions = rt.last_frame_regions()
        assert regions == ["Update Indirect Buffer", "GPU Culling", "Update Indirect Buffer", "GPU Culling", "DepthPrepass QueueTag:Opaque",
                           "DepthPrepass QueueTag:Masked"], regions
        same(depth, scene.raw, "DepthBuffer of the prepass-only graph")
        # a Masked prepass begun from the Opaque depth alone leaves the opaque depth in every hole of the checker
        raw, opaque = scene.raw.cpu().numpy(), scene.opaque.cpu().numpy()
        assert ((raw != opaque).sum() > 300) and (raw >= opaque).all()
    finally:
        rt.close()


def test_a_shader_without_a_route_under_draw_indexed_indirect_is_the_frames_status(ctx, scene):
    """Runtime.draw_indexed_indirect records and submits ONE depth-only pass of one DrawIndexedIndirect with a material of the given shader, as a node would:
    a routed shader draws, any other launches nothing and is SAILOR_HIP_ERR_UNSUPPORTED.  The driver keeps the last failing status (m_lastDispatchStatus is
    never reset, as everywhere in this driver), so the process_frame() that follows -- itself a clean frame -- returns that left-over status: what is shown is
    that the refusal reaches the caller of process_frame(), not a refusal inside the frame."""
    main, depth = scene.sky.clone(), garbage_depth(scene)
    rt = scene.runtime_from(PREPASS_ONLY, main, depth)
    try:
        assert rt.process_frame() == 0
        rt.wait_idle()
        scratch = garbage_depth(scene)
        assert rt.draw_indexed_indirect("Shaders/DepthOnly.shader", scratch) == 0
        torch.cuda.synchronize()
        assert (scratch.cpu().numpy() != 0.75).any()
        before, _ = rt.launch_log(0)
        for shader in ("Shaders/ShadowCaster.shader", "Shaders/Gizmo.shader", "Shaders/ImGuiUI.shader", "Shaders/Blit.shader"):
            assert rt.draw_indexed_indirect(shader, scratch) == UNSUPPORTED, shader
        after, _ = rt.launch_log(0)
        assert after == before   # nothing was launched for them
        status = rt.process_frame()
        rt.wait_idle()
        assert status == UNSUPPORTED   # the sticky status of the refused submissions above
    finally:
        rt.close()
