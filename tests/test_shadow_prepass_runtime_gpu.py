"""The ShadowPrepass and Clear nodes through the C++ host mirror: a `.renderer` text of its own -- Clear DepthBuffer, Clear Main, ShadowPrepass, LinearizeDepth,
LightCulling, RenderScene -- over tests/shadow_prepass_cases.py's scene (a ground in four strips, a few boxes, one directional light), once with an EVSM light
and once with a PCF light.
  (a) after the frame every cascade map equals the C-ABI sequence bit for bit: sailor_hip_raster_depth over the id list NumPy derives from the pass's mask, batch
      by batch, sailor_hip_shadow_resolve, sailor_hip_evsm_blur where the node blurs (every EVSM pass); one cascade at 64 x 64 also against oracle.raster_depth;
  (b) `lightsMatrices` equals the host's cascade matrices x light matrix bit for bit;
  (c) `Main` equals, bit for bit, the `Main` of a second runtime that is handed the same maps and matrices through set_shadow_maps and has no ShadowPrepass entry;
  (d) a second, unchanged frame launches nothing from raster.hip, shadow_blur.hip or shadow_instances.hip and leaves `Main` as it was; the camera moved by 16 units
      re-renders;
  (e) with the box that cascades 1 and 2 share, cascade 2's map equals the map drawn from its un-deduplicated overlap set -- what m_internalCommandsList is for;
  (f) with the scene taken away `Main` is the clear colour as the target stores it and DepthBuffer is 0 everywhere;
  (g) a runtime that did not opt in reports both entries as skipped and renders what it renders today.
The depth attachment RenderScene tests against is the caller's prepass depth (as in tests/test_surface_runtime_gpu.py); the Clear of DepthBuffer is checked on its own,
(f)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import shadow_prepass_cases as sc
import shadow_prepass_ref as ref
from oracle import oracle
from sailor_amd import _lib, host
from sailor_amd.forward_plus import evsm_blur, linearize_depth, raster_depth, shadow_extract_positions, shadow_resolve, upload_textures
from sailor_amd.runtime_binding import Runtime

pytestmark = pytest.mark.gpu
PCF, EVSM = ref.PCF, ref.EVSM
SIZES = (64, 128, 256, 64)            # the cascade maps' resolutions in these tests
CLEAR_COLOR = [1.502, 2.08, 2.61, 2.5]   # DefaultRenderer.renderer:136
SHADOW_KERNELS = ("k_raster", "k_shadow_resolve", "k_evsm", "k_shadow_gather", "k_shadow_positions")   # raster.hip, shadow_blur.hip, shadow_instances.hip


def renderer(shadow_prepass: bool = True, clears: bool = True, scene_depth: str = "SceneDepth") -> str:
    clear = f"""- name: Clear
  float:
  - clearDepth: 0
  - clearStencil: 0
  renderTargets:
  - target: DepthBuffer

- name: Clear
  vec4:
  - clearColor: {CLEAR_COLOR}
  renderTargets:
  - target: Main

""" if clears else ""
    shadows = "- name: ShadowPrepass\n\n" if shadow_prepass else ""
    return f"""---
frame:
{clear}{shadows}- name: LinearizeDepth
  renderTargets:
  - depthStencil: {scene_depth}
  - target: LinearDepth

- name: LightCulling
  renderTargets:
  - depthStencil: LinearDepth

- name: RenderScene
  string:
  - Tag: Opaque
  renderTargets:
  - color: Main
  - depthStencil: {scene_depth}
"""


def kernel_file_launches(names):
    return [n for n in names if n.startswith(SHADOW_KERNELS)]


def same(got, want, what=""):
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    w = want.cpu().numpy() if torch.is_tensor(want) else want
    if g.dtype == np.float16:
        g, w = g.view(np.uint16), w.view(np.uint16)
    else:
        g, w = g.view(np.uint32), w.view(np.uint32)
    np.testing.assert_array_equal(g, w, err_msg=what)


def download(ptr, shape, dtype):
    out = np.empty(shape, dtype)
    lib, ctx = _lib.load(), C.c_void_p()
    _lib.check(lib.sailor_hip_context_create(0, None, 0, C.byref(ctx)), "context_create")
    try:
        _lib.check(lib.sailor_hip_buffer_download(ctx, out.ctypes.data, ptr, 0, out.nbytes), "buffer_download", ctx)
    finally:
        lib.sailor_hip_context_destroy(ctx)
    return out


class Scene:
    def __init__(self, ctx, shared: bool):
        self.L = L = sc.layout(shared)
        self.cam = sc.camera()
        dev = ctx.device
        self.vertices, self.indices = torch.from_numpy(L.vertices).to(dev), torch.from_numpy(L.indices.view(np.int32)).to(dev)
        self.instances, self.materials = torch.from_numpy(L.instances.view(np.uint8).copy()).to(dev), torch.from_numpy(L.materials.view(np.uint8).copy()).to(dev)
        self.textures, self.num_textures, self.keep = upload_textures(ctx, L.textures, L.srgb)
        self.world_aabb = torch.from_numpy(L.world_aabb).to(dev)
        self.positions = shadow_extract_positions(ctx, self.vertices)
        self.models = torch.from_numpy(np.ascontiguousarray(L.instances["model"])).to(dev)
        ctx.synchronize()
        np.testing.assert_array_equal(self.positions.cpu().numpy().view(np.uint32), np.ascontiguousarray(L.vertices[:, 2:5]).view(np.uint32))   # the extraction kernel
        self.sky = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, (sc.H, sc.W, 4)).astype(np.float32)).to(dev)

    def prepass(self, ctx, cam):
        """the caller's depth prepass of the scene (DepthOnly.shader, back faces culled) -> raw depth [H, W]"""
        raw = torch.zeros((sc.H, sc.W), dtype=torch.float32, device=ctx.device)
        for count, n, first_index, vertex_offset, first_instance in self.L.batches.tolist():
            _lib.check(ctx._lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(cam.frame), self.positions.data_ptr() + 12 * vertex_offset, self.indices.data_ptr() + 4 * first_index,
                                                               count // 3, self.models.data_ptr() + 64 * first_instance, None, n, sc.W, sc.H, raw.data_ptr(), _lib.RASTER_CULL_BACK, None),
                       "sailor_hip_raster_depth_camera", ctx.handle)
        ctx.synchronize()
        return raw

    def draw_map(self, ctx, light_matrix, mask, size, fmt, blur):
        """one cascade map through the C-ABI: the ids NumPy derives from the mask, batch by batch, resolve, blur"""
        ids = np.nonzero(np.unpackbits(np.ascontiguousarray(mask, np.uint64).view(np.uint8), bitorder="little")[: self.L.num_instances])[0].astype(np.uint32)
        depth = torch.zeros((size, size), dtype=torch.float32, device=ctx.device)
        for count, n, first_index, vertex_offset, first_instance in self.L.batches.tolist():
            own = ids[(ids >= first_instance) & (ids < first_instance + n)]
            if len(own):
                raster_depth(ctx, light_matrix, self.positions[vertex_offset:], self.indices[first_index:first_index + count], self.models, size, size,
                             instance_ids=torch.from_numpy(own.view(np.int32)).to(ctx.device), depth=depth, cull_back=True)
        out = shadow_resolve(ctx, depth, fmt)
        if blur:
            evsm_blur(ctx, out, 2, 5, torch.empty_like(out))
        ctx.synchronize()
        return out, depth, ids

    def runtime(self, ctx, text, light_type, cam, main, scene_depth, enable=True, casters=True, with_scene=True):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        rt.set_camera(cam)
        if enable:
            rt.enable_node("ShadowPrepass")
            rt.enable_node("Clear")
        loaded = rt.load_renderer(text)
        rt.set_color_target("Main", main)
        depth_buffer = torch.full((sc.H, sc.W), 0.75, dtype=torch.float32, device=ctx.device)
        linear = torch.zeros((sc.H, sc.W), dtype=torch.float32, device=ctx.device)
        rt.set_render_target("DepthBuffer", depth_buffer)
        rt.set_render_target("SceneDepth", scene_depth)
        rt.set_render_target("LinearDepth", linear)
        rt.set_depth(linear)
        rt.set_raw_depth(scene_depth)
        index = rt.add_light(0, light_type, sc.LIGHT_POSITION, [0.0, -1.0, 0.0], [3.0, 3.0, 3.0], [100.0, 100.0, 100.0])
        rt.set_light_rotation(index, sc.LIGHT_ROTATION)
        rt.tick_lights()
        if with_scene:
            rt.set_scene(self.vertices, self.indices, self.instances, self.materials, self.textures, self.num_textures, self.L.batches)
            rt.set_scene_tags(["Opaque", "Opaque"], [0, 0])
            if casters:
                rt.set_caster_data(self.world_aabb, self.L.last_changed_frames, resolutions=SIZES, trace="flat")
        rt.keep = (main, scene_depth, depth_buffer, linear)   # what the runtime was handed stays alive as long as it does
        return rt, loaded, depth_buffer, linear


def frame_launches(rt):
    before, _ = rt.launch_log(0)
    status = rt.process_frame()
    rt.wait_idle()
    after, names = rt.launch_log(16)
    n = min(after - before, 16)
    return status, names[len(names) - n:] if n else [], after - before


@pytest.fixture(scope="module")
def scene(ctx):
    return Scene(ctx, shared=False)


@pytest.fixture(scope="module")
def shared_scene(ctx):
    return Scene(ctx, shared=True)


@pytest.mark.parametrize("light_type", [EVSM, PCF])
def test_maps_matrices_main_and_change_tracking(ctx, scene, light_type):
    L, cam = scene.L, scene.cam
    raw = scene.prepass(ctx, cam)
    main = scene.sky.clone()
    rt, loaded, depth_buffer, _ = scene.runtime(ctx, renderer(), light_type, cam, main, raw)
    try:
        assert loaded[1] == 0, loaded   # nothing skipped: both classes were created
        status, names, launched = frame_launches(rt)
        assert status == 0, (status, names)
        assert rt.last_frame_regions()[:3] == ["Clear", "Clear", "ShadowPrepass"], rt.last_frame_regions()
        # the passes LightingECS planned: the restatement over the CPU oracle's overlap sets
        planes = sc.cascade_planes(cam)
        view = (0, (*cam.world[12:15], 1.0), (0.0, 0.0, 0.0, 1.0), (*sc.LIGHT_POSITION, 0.0), tuple(sc.LIGHT_ROTATION))
        want_passes = ref.Planner().frame([light_type], [view], L.num_instances, oracle.csm_caster_masks(L.world_aabb, planes)[None], L.last_changed_frames, None, L.batch_ranges)
        passes = rt.shadow_passes(L.num_instances)
        assert [(p["cascade"], p["shadow_type"], p["casters"], p["dependencies"]) for p in passes] == \
               [(p["cascade"], p["shadow_type"], p["casters"], p["dependencies"]) for p in want_passes]
        assert [p["shadow_type"] for p in passes] == [light_type, PCF, PCF, PCF] and all(p["casters"] >= 3 for p in passes)
        for p, w in zip(passes, want_passes):
            np.testing.assert_array_equal(p["mask"], w["mask"])
        # (b) lightsMatrices
        lm = sc.lights_matrices(cam)
        same(rt.lights_matrices(), lm, "lightsMatrices")
        # (a) every cascade map, bit for bit
        maps, formats = [], []
        for k, p in enumerate(passes):
            ptr, size, fmt = rt.csm_shadow_map(k)
            evsm = p["shadow_type"] == EVSM
            assert size == SIZES[k] and fmt == (_lib.SHADOWMAP_RGBA32F if evsm else _lib.SHADOWMAP_R16F)
            want, depth, ids = scene.draw_map(ctx, lm[k], p["mask"], size, fmt, blur=evsm)
            got = download(ptr, (size, size, 4) if evsm else (size, size), np.float32 if evsm else np.float16)
            same(got, want, f"cascade {k}")
            assert (depth.cpu().numpy() > 0).mean() > 0.02, k   # something was drawn
            if k == 3:   # 64 x 64: the depth behind the map against the CPU oracle
                want_depth = np.zeros((size, size), np.float32)
                for count, n, first_index, vertex_offset, first_instance in L.batches.tolist():
                    own = ids[(ids >= first_instance) & (ids < first_instance + n)]
                    if len(own):
                        want_depth = oracle.raster_depth(lm[k], L.vertices[vertex_offset:, 2:5], L.indices[first_index:first_index + count], L.instances["model"], size, size,
                                                         instance_ids=own, depth=want_depth, cull_back=True)
                same(depth, want_depth, "cascade 3's depth against oracle.raster_depth")
            maps.append(want); formats.append(fmt)
        first_main = main.clone()
        assert torch.isfinite(first_main).all()
        # (d) an unchanged frame records nothing from the three files and leaves Main as it was
        status, names, launched = frame_launches(rt)
        assert status == 0, status
        assert kernel_file_launches(names) == [], names
        assert rt.shadow_passes() == []
        same(main, first_main, "Main of the unchanged frame")
        # ... the camera moved by 16 units re-renders every cascade
        moved = sc.camera((16.0, 150.0, 0.0))
        rt.set_camera(moved)
        assert rt.process_frame() == 0
        rt.wait_idle()
        assert [p["cascade"] for p in rt.shadow_passes()] == [0, 1, 2, 3]
        same(rt.lights_matrices(), sc.lights_matrices(moved), "lightsMatrices of the moved camera")
    finally:
        rt.close()
    # (c) the hand-in path: a runtime without the ShadowPrepass entry, given the same maps and matrices
    second = scene.sky.clone()
    rt2, loaded2, _, _ = scene.runtime(ctx, renderer(shadow_prepass=False), light_type, cam, second, raw, casters=False)
    try:
        assert loaded2[1] == 0, loaded2
        rt2.set_shadow_maps(maps, formats, lm)
        assert rt2.process_frame() == 0
        rt2.wait_idle()
        same(second, first_main, "Main through set_shadow_maps")
    finally:
        rt2.close()
    covered = raw.cpu().numpy() > 0
    assert 0.2 < covered.mean() < 0.99
    got = first_main.cpu().numpy()
    np.testing.assert_array_equal(got[~covered].view(np.uint32), np.broadcast_to(np.float32(CLEAR_COLOR), got.shape)[~covered].view(np.uint32))   # the Clear of Main


def test_dependency_passes_draw_what_the_removal_took_out(ctx, shared_scene):
    L, cam = shared_scene.L, shared_scene.cam
    shared = sc.PAD_INSTANCES + L.num_boxes - 1
    raw = shared_scene.prepass(ctx, cam)
    main = shared_scene.sky.clone()
    rt, loaded, _, _ = shared_scene.runtime(ctx, renderer(), PCF, cam, main, raw)
    try:
        assert rt.process_frame() == 0
        rt.wait_idle()
        passes = rt.shadow_passes(L.num_instances)
        assert [p["dependencies"] for p in passes] == [[], [], [1], []]
        assert ref.bits(passes[1]["mask"], L.num_instances)[shared] and not ref.bits(passes[2]["mask"], L.num_instances)[shared]
        lm = sc.lights_matrices(cam)
        overlap = oracle.csm_caster_masks(L.world_aabb, sc.cascade_planes(cam))
        assert ref.bits(overlap[1], L.num_instances)[shared] and ref.bits(overlap[2], L.num_instances)[shared]
        ptr, size, fmt = rt.csm_shadow_map(2)
        got = download(ptr, (size, size), np.float16)
        # (e) cascade 2's map = the map of its own set plus pass 1's set (what the node draws) = the map of the un-deduplicated overlap set: what pass 1 holds
        # beyond the shared box lies outside cascade 2's frustum and leaves no fragment
        both, _, _ = shared_scene.draw_map(ctx, lm[2], passes[2]["mask"] | passes[1]["mask"], size, fmt, blur=False)
        whole, _, _ = shared_scene.draw_map(ctx, lm[2], overlap[2], size, fmt, blur=False)
        alone, _, _ = shared_scene.draw_map(ctx, lm[2], passes[2]["mask"], size, fmt, blur=False)
        same(got, both, "cascade 2 with its dependency")
        same(got, whole, "cascade 2 against the un-deduplicated overlap set")
        assert (alone.cpu().numpy().view(np.uint16) != got.view(np.uint16)).any()   # the shared box does show in cascade 2
        # the reference's second frame over a shared caster: cascade 1 is not re-rendered, cascade 2 takes the box back and is drawn again, alone (the CPU test)
        assert rt.process_frame() == 0
        rt.wait_idle()
        again = rt.shadow_passes(L.num_instances)
        assert [(p["cascade"], p["dependencies"]) for p in again] == [(2, [])] and ref.bits(again[0]["mask"], L.num_instances)[shared]
        same(download(ptr, (size, size), np.float16), whole, "cascade 2 redrawn from its own list")
        status, names, launched = frame_launches(rt)
        assert status == 0 and rt.shadow_passes() == [] and kernel_file_launches(names) == [], names
    finally:
        rt.close()


def test_clear_alone_main_is_the_clear_colour_and_depth_buffer_is_zero(ctx, scene):
    main = scene.sky.clone()
    raw = torch.zeros((sc.H, sc.W), dtype=torch.float32, device=ctx.device)
    rt, loaded, depth_buffer, _ = scene.runtime(ctx, renderer(), EVSM, scene.cam, main, raw, with_scene=False)
    try:
        assert loaded[1] == 0
        assert (depth_buffer.cpu().numpy() == 0.75).all()
        status, names, launched = frame_launches(rt)
        assert status == 0, (status, names)
        assert kernel_file_launches(names) == []   # no scene, no caster data: ShadowPrepass returns early
        assert rt.last_frame_regions()[:2] == ["Clear", "Clear"] and "ShadowPrepass" not in rt.last_frame_regions()
        got = main.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), np.broadcast_to(np.float32(CLEAR_COLOR), got.shape).view(np.uint32))   # fp32 channels: the colour itself
        assert (depth_buffer.cpu().numpy().view(np.uint32) == 0).all()
    finally:
        rt.close()


def test_without_the_opt_in_both_entries_are_skipped_and_the_frame_is_todays(ctx, scene):
    cam = scene.cam
    raw = scene.prepass(ctx, cam)
    runs = {}
    for text, enable in ((renderer(), False), (renderer(shadow_prepass=False, clears=False), False)):
        main = scene.sky.clone()
        rt, loaded, depth_buffer, _ = scene.runtime(ctx, text, PCF, cam, main, raw, enable=enable, casters=False)
        try:
            runs[text] = (loaded, main, depth_buffer)
            status, names, launched = frame_launches(rt)
            assert status == 0 and kernel_file_launches(names) == [], (status, names)
            assert "Clear" not in rt.last_frame_regions() and "ShadowPrepass" not in rt.last_frame_regions()
        finally:
            rt.close()
    (with_entries, main_a, depth_a), (without, main_b, depth_b) = runs.values()
    assert with_entries[1] == 3 and without[1] == 0 and with_entries[0] == without[0] == 3   # Clear, Clear, ShadowPrepass reported as not implemented
    same(main_a, main_b, "Main with the three entries skipped")
    assert (depth_a.cpu().numpy() == 0.75).all()   # nobody cleared DepthBuffer
    covered = raw.cpu().numpy() > 0
    got = main_a.cpu().numpy()
    np.testing.assert_array_equal(got[~covered].view(np.uint32), scene.sky.cpu().numpy()[~covered].view(np.uint32))   # nobody cleared Main
