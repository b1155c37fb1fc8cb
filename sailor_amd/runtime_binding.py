"""ctypes binding of sailor_amd/runtime/libsailor_runtime.so -- the C++ host mirror (RHI / FrameGraph / GraphicsDriver/HIP / ECS).

The harness drives the path the way the engine does: a Renderer with the HIP backend, a frame graph built from node NAMES
("LightCulling", "RenderScene"), a scene snapshot, `RHIFrameGraph::Process` per frame.  Used by the tests; device memory is
torch's."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _lib

LIB_PATH = Path(__file__).resolve().parent / "runtime" / "libsailor_runtime.so"
_rt = None


def load() -> C.CDLL:
    global _rt
    if _rt is None:
        _lib.load()  # torch's HIP runtime + libsailor_hip.so first
        if not LIB_PATH.exists():
            raise _lib.SailorHipError(-2, "runtime", f"{LIB_PATH} is missing: make -C sailor_amd/runtime")
        rt = C.CDLL(str(LIB_PATH))
        P = C.c_void_p
        rt.sailor_rt_create.restype = P
        rt.sailor_rt_create.argtypes = [C.c_int, P, C.c_int, C.POINTER(C.c_int)]
        rt.sailor_rt_destroy.argtypes = [P]
        rt.sailor_rt_node_registered.argtypes = [C.c_char_p]
        rt.sailor_rt_build_graph.argtypes = [P, C.POINTER(C.c_char_p), C.c_int]
        rt.sailor_rt_set_camera.argtypes = [P, P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
        rt.sailor_rt_set_lights.argtypes = [P, P, C.c_int]
        rt.sailor_rt_add_light.argtypes = [P, C.c_uint32, C.c_uint32, P, P, P, P, P]
        rt.sailor_rt_tick_lights.argtypes = [P]
        rt.sailor_rt_update_light.argtypes = [P, C.c_int, P, P, P, P, P]
        rt.sailor_rt_set_light_state.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong]
        rt.sailor_rt_light_uploads.argtypes = [P, P, C.c_int]
        rt.sailor_rt_total_num_lights.restype = C.c_uint32
        rt.sailor_rt_total_num_lights.argtypes = [P]
        rt.sailor_rt_set_depth.argtypes = [P, P, C.c_int, C.c_int]
        rt.sailor_rt_set_raw_depth.argtypes = [P, P, C.c_int, C.c_int]
        rt.sailor_rt_set_surface.argtypes = [P, P, P, C.c_int, C.c_int]
        rt.sailor_rt_set_shadow_maps.argtypes = [P, P, P, P, P]
        rt.sailor_rt_set_ibl.argtypes = [P, P, C.c_int, P, C.c_int, C.c_int, P, C.c_int, C.c_int, P, C.c_int, C.c_int]
        rt.sailor_rt_blur_shadow_map.argtypes = [P, P, P, C.c_int, C.c_float, C.c_float]
        rt.sailor_rt_set_sky_cubemap.argtypes = [P, P, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int]
        rt.sailor_rt_sky_set_params.argtypes = [P, P, C.c_int]
        rt.sailor_rt_sky_state.argtypes = [P, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_sky_set_cloud_textures.argtypes = [P, P, C.c_int, C.c_int, P, C.c_int, P, C.c_int]
        rt.sailor_rt_sky_set_stars.argtypes = [P, P, C.c_int]
        rt.sailor_rt_set_particles.argtypes = [P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, C.c_uint32,
                                               C.c_int, C.c_int]
        rt.sailor_rt_particles_buffers.argtypes = [P, C.POINTER(P), C.POINTER(C.c_uint32), C.POINTER(P), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_set_environment_map.argtypes = [P, P, C.c_int, C.c_int, C.c_int, C.c_int]
        rt.sailor_rt_sampler.restype = P
        rt.sailor_rt_sampler.argtypes = [P, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_build_depth_highz.argtypes = [P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(P)]
        rt.sailor_rt_parse_renderer.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
        rt.sailor_rt_parse_world.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        rt.sailor_rt_load_world.argtypes = [P, C.c_char_p, C.c_int, C.c_int, P, P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_load_renderer.argtypes = [P, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_render_target.restype = P
        rt.sailor_rt_render_target.argtypes = [P, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_set_render_target.argtypes = [P, C.c_char_p, P, C.c_int, C.c_int]
        rt.sailor_rt_set_sampler.argtypes = [P, C.c_char_p, P, C.c_int, C.c_int]
        rt.sailor_rt_set_color_target.argtypes = [P, C.c_char_p, P, C.c_int, C.c_int]
        rt.sailor_rt_set_time.argtypes = [P, C.c_float, C.c_float]
        rt.sailor_rt_enable_node.argtypes = [P, C.c_char_p]
        rt.sailor_rt_enable_shader.argtypes = [P, C.c_char_p]
        rt.sailor_rt_launch_log.argtypes = [P, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p), C.c_int]
        rt.sailor_rt_set_color_target_chain.argtypes = [P, C.c_char_p, P, C.c_int, C.c_int, C.c_int]
        rt.sailor_rt_eye_adaptation_state.argtypes = [P, C.POINTER(P), C.POINTER(P)]
        rt.sailor_rt_shadow_pass.argtypes = [P, C.POINTER(C.c_float), P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, C.c_uint32, P, C.c_int, C.c_int, C.c_float, C.c_float]
        rt.sailor_rt_gpu_culling.argtypes = [P, P, C.c_uint32, C.c_uint32, P, C.c_uint32]
        rt.sailor_rt_set_scene.argtypes = [P, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, P, C.c_int]
        rt.sailor_rt_set_scene_texture_levels.argtypes = [P, P, C.c_int]
        rt.sailor_rt_generate_texture_mips.argtypes = [P, P, C.c_int, C.c_int, C.c_int, P, C.c_size_t]
        rt.sailor_rt_set_scene_targets.argtypes = [P, P, P, C.c_int, C.c_int]
        rt.sailor_rt_set_scene_tags.argtypes = [P, C.c_char_p, P, C.c_int]
        rt.sailor_rt_set_scene_shaders.argtypes = [P, P, C.c_int]
        rt.sailor_rt_set_scene_blend.argtypes = [P, P, P, C.c_int]
        rt.sailor_rt_set_transparent_layers.argtypes = [P, C.c_int]
        rt.sailor_rt_set_transparent_mode.argtypes = [P, C.c_int]
        rt.sailor_rt_transparent_overflow.argtypes = [P]
        rt.sailor_rt_transparent_overflow.restype = C.c_longlong
        rt.sailor_rt_process_frame.argtypes = [P]
        rt.sailor_rt_capture_next_frame.argtypes = [P, C.c_char_p, P, C.c_int, P, C.c_size_t]
        rt.sailor_rt_capture_result.argtypes = [P, P, C.c_int]
        rt.sailor_rt_node_indirect_commands.argtypes = [P, C.c_int, P, C.c_int]
        rt.sailor_rt_draw_indexed_indirect.argtypes = [P, C.c_char_p, P, C.c_int, C.c_int]
        rt.sailor_rt_last_frame_regions.argtypes = [P, C.c_char_p, C.c_int]
        for shape in ("line", "aabb", "arrow"):
            getattr(rt, f"sailor_rt_debug_draw_{shape}").argtypes = [P, P, P, P, C.c_float]
        rt.sailor_rt_debug_draw_frustum.argtypes = [P, P, P, C.c_float]
        rt.sailor_rt_debug_draw_origin.argtypes = [P, P, P, C.c_float, C.c_float]
        rt.sailor_rt_debug_draw_sphere.argtypes = [P, P, C.c_float, P, C.c_float]
        rt.sailor_rt_debug_tick.argtypes = [P, C.c_float]
        rt.sailor_rt_debug_vertices.argtypes = [P, P, C.c_int]
        rt.sailor_rt_set_ui_draw_data.argtypes = [P, P, P, P, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, P, C.c_uint32, P, C.c_int, C.c_int]
        rt.sailor_rt_process_frame_overwriting_lists.argtypes = [P, P, C.c_size_t, P, C.c_size_t]
        rt.sailor_rt_set_frame_split.argtypes = [P, C.c_int, C.c_int, P]
        rt.sailor_rt_exchange_light_lists.argtypes = [P, P, C.c_size_t, P, C.c_size_t]
        rt.sailor_rt_wait_idle.argtypes = [P]
        rt.sailor_rt_buffer.restype = P
        rt.sailor_rt_buffer.argtypes = [P, C.c_char_p, C.POINTER(C.c_size_t)]
        rt.sailor_rt_ecs_sweep.argtypes = [P, P, P, P, C.c_uint32, P, C.c_uint32, C.POINTER(P), C.POINTER(P), C.POINTER(P)]
        rt.sailor_rt_ecs_sweep_traced.argtypes = [P, P, P, P, C.c_uint32, P, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(P), C.POINTER(P), C.POINTER(P),
                                                  C.POINTER(P)]
        rt.sailor_rt_set_caster_data.argtypes = [P, P, C.c_uint32, P, P, P, C.c_uint32, C.c_uint32]
        rt.sailor_rt_set_light_rotation.argtypes = [P, C.c_int, P]
        rt.sailor_rt_shadow_passes.argtypes = [P, P, P, C.c_uint32, C.c_int]
        rt.sailor_rt_csm_shadow_map.restype = P
        rt.sailor_rt_csm_shadow_map.argtypes = [P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        rt.sailor_rt_lights_matrices.argtypes = [P, P]
        rt.sailor_rt_csm_planner_create.restype = P
        rt.sailor_rt_csm_planner_destroy.argtypes = [P]
        rt.sailor_rt_csm_planner_frame.argtypes = [P, C.c_uint32, P, P, C.c_uint32, P, P, P, P, C.c_uint32, C.c_uint32, P, P, P]
        _rt = rt
    return _rt


class CsmPlanner:
    """LightingECS's pass planning without a device (sailor_rt_csm_planner_*): the host half of PrepareCSMPasses over overlap sets the caller supplies, with
    the snapshots carried from frame to frame.  frame() returns one dict per pass: light, cascade (m_lighMatrixIndex), shadow_type, casters, dependencies
    (m_internalCommandsList), mask (uint64 words) and runs (uint32 [batches, 2] = count, offset of the batch's run in the pass's slice of the SSBO)."""

    def __init__(self):
        self.rt = load()
        self.h = self.rt.sailor_rt_csm_planner_create()

    def close(self):
        if self.h:
            self.rt.sailor_rt_csm_planner_destroy(self.h)
            self.h = None

    def frame(self, light_shadow_types, views, num_instances: int, overlap_masks, last_changed_frame, cast_shadows=None, batch_ranges=()):
        n = len(light_shadow_types)
        words = (num_instances + 63) // 64
        types = np.ascontiguousarray(light_shadow_types, np.uint32)
        view_array = (_lib.CsmView * max(n, 1))(*views)
        masks = np.ascontiguousarray(overlap_masks, np.uint64).reshape(n, 4, words)
        frames = np.ascontiguousarray(last_changed_frame, np.uint64)
        assert len(frames) == num_instances
        cast = None if cast_shadows is None else np.ascontiguousarray(cast_shadows, np.uint64)
        assert cast is None or len(cast) == words
        ranges = np.ascontiguousarray(batch_ranges, np.uint32).reshape(-1, 2)
        cap = 4 * max(n, 1)
        info, out_masks, runs = np.zeros((cap, 8), np.uint32), np.zeros((cap, max(words, 1)), np.uint64), np.zeros((cap, max(len(ranges), 1), 2), np.uint32)
        count = self.rt.sailor_rt_csm_planner_frame(self.h, n, types.ctypes.data, view_array, num_instances, masks.ctypes.data, frames.ctypes.data,
                                                    None if cast is None else cast.ctypes.data, ranges.ctypes.data if len(ranges) else None, len(ranges), cap,
                                                    info.ctypes.data, out_masks.ctypes.data, runs.ctypes.data)
        if count < 0:
            raise ValueError("sailor_rt_csm_planner_frame refused its arguments")
        return [{"light": int(i[0]), "cascade": int(i[1]), "shadow_type": int(i[2]), "casters": int(i[3]), "dependencies": [int(d) for d in i[5:5 + int(i[4])]],
                 "mask": out_masks[p, :words].copy(), "runs": runs[p, :len(ranges)].copy()} for p, i in enumerate(info[:count])]


def parse_world(text: str):
    """WorldPrefab::Deserialize + World::Instantiate of a `.world` text (no device needed): (number of game objects, summary string)"""
    rt = load()
    buf = C.create_string_buffer(1 << 16)
    n = rt.sailor_rt_parse_world(text.encode(), buf, len(buf))
    if n < 0:
        raise ValueError(buf.value.decode())
    return n, buf.value.decode()


def parse_renderer(text: str, viewport_width: int, viewport_height: int):
    """FrameGraphAsset::Deserialize of a `.renderer` text (no device needed): (number of frame nodes, summary string); raises on a parse error"""
    rt = load()
    buf = C.create_string_buffer(1 << 16)
    n = rt.sailor_rt_parse_renderer(text.encode(), viewport_width, viewport_height, buf, len(buf))
    if n < 0:
        raise ValueError(buf.value.decode())
    return n, buf.value.decode()


class Runtime:
    def __init__(self, device_index: int = 0, stream_handle: int = 0):
        self.rt = load()
        st = C.c_int(0)
        self.h = self.rt.sailor_rt_create(device_index, C.c_void_p(stream_handle), 0, C.byref(st))
        if not self.h:
            raise _lib.SailorHipError(st.value, "sailor_rt_create")

    def call(self, name: str, *args):
        """the checked call of the harness entry `name`, which takes this runtime first: a status other than 0 raises under the entry's name"""
        _lib.check(getattr(self.rt, name)(self.h, *args), name)

    def close(self):
        if self.h:
            self.rt.sailor_rt_destroy(self.h)
            self.h = None

    def build_graph(self, names):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        if self.rt.sailor_rt_build_graph(self.h, arr, len(names)) != 0:
            raise ValueError(f"unknown frame graph node in {names}")

    def set_camera(self, cam):
        w = np.ascontiguousarray(cam.world, np.float32)
        self.rt.sailor_rt_set_camera(self.h, w.ctypes.data, cam.fov, cam.aspect, cam.z_near, cam.z_far, cam.width, cam.height)

    def set_lights(self, lights: np.ndarray):
        raw = np.ascontiguousarray(lights).view(np.uint8)
        self.rt.sailor_rt_set_lights(self.h, raw.ctypes.data, len(lights))

    @staticmethod
    def _f3(v):
        return None if v is None else np.ascontiguousarray(v, np.float32).ctypes.data_as(C.c_void_p)

    def add_light(self, light_type: int, shadow_type: int, position, direction, intensity, bounds, cut_off_degrees=None) -> int:
        """register one light as a component (LightData; cut-off in degrees); packed by the next tick_lights()"""
        keep = [np.ascontiguousarray(v, np.float32) for v in (position, direction, intensity, bounds)]
        cut = np.ascontiguousarray(cut_off_degrees, np.float32) if cut_off_degrees is not None else None
        return self.rt.sailor_rt_add_light(self.h, light_type, shadow_type, *[k.ctypes.data for k in keep], cut.ctypes.data if cut is not None else None)

    def update_light(self, index: int, position=None, direction=None, intensity=None, bounds=None, cut_off_degrees=None):
        """new parameters for one light + MarkDirty"""
        keep = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (position, direction, intensity, bounds, cut_off_degrees)]
        assert self.rt.sailor_rt_update_light(self.h, index, *[None if k is None else k.ctypes.data for k in keep]) == 0

    def set_light_state(self, index: int, active=None, dirty=None, mobility=None, owner_frame_last_change=None):
        """TComponent::SetActive / MarkDirty, the owner's mobility (0 static, 1 stationary, 2 dynamic) and GameObject::GetFrameLastChange"""
        enc = lambda v: -1 if v is None else int(v)
        assert self.rt.sailor_rt_set_light_state(self.h, index, enc(active), enc(dirty), enc(mobility), enc(owner_frame_last_change)) == 0

    def tick_lights(self):
        """LightingECS::Tick + FillLightingData; returns the copies it recorded as [(first record slot, record count)]"""
        self.rt.sailor_rt_tick_lights(self.h)
        buf = np.zeros(2 * 4096, np.uint32)
        n = self.rt.sailor_rt_light_uploads(self.h, buf.ctypes.data, 4096)
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(min(n, 4096))]

    def total_num_lights(self) -> int:
        return self.rt.sailor_rt_total_num_lights(self.h)

    def set_depth(self, depth_tensor):
        self.rt.sailor_rt_set_depth(self.h, depth_tensor.data_ptr(), depth_tensor.shape[1], depth_tensor.shape[0])

    def set_raw_depth(self, raw_tensor):
        """after set_depth: the LinearizeDepth node reads this and writes the tensor given to set_depth"""
        self.rt.sailor_rt_set_raw_depth(self.h, raw_tensor.data_ptr(), raw_tensor.shape[1], raw_tensor.shape[0])

    def set_ibl(self, irradiance, env_chain, env_size, env_levels, lut, ao):
        """device tensors: irradiance [6,S,S,4], env mip chain (flat), lut [H,W,2], ao [H,W] or None"""
        self.rt.sailor_rt_set_ibl(self.h, irradiance.data_ptr(), irradiance.shape[1], env_chain.data_ptr(), env_size, env_levels,
                                  lut.data_ptr(), lut.shape[1], lut.shape[0], ao.data_ptr() if ao is not None else None,
                                  ao.shape[1] if ao is not None else 0, ao.shape[0] if ao is not None else 0)

    def blur_shadow_map(self, moments, temp, radius_umbra, radius_penumbra):
        """the blur section of ShadowPrepassNode::Process over a float32 [S, S, 4] device tensor, in place"""
        return self.rt.sailor_rt_blur_shadow_map(self.h, moments.data_ptr(), temp.data_ptr(), moments.shape[0], radius_umbra, radius_penumbra)

    def set_sky_cubemap(self, chain, size, levels, irradiance_size=0, ao=None):
        """publish the raw environment cube (flat RGBA32F mip chain, device tensor) as "g_skyCubemap" and mark the Environment node dirty"""
        return self.rt.sailor_rt_set_sky_cubemap(self.h, chain.data_ptr(), size, levels, irradiance_size, ao.data_ptr() if ao is not None else None,
                                                 ao.shape[1] if ao is not None else 0, ao.shape[0] if ao is not None else 0)

    def sky_set_params(self, params, mark_dirty: bool = False) -> int:
        """replace the Sky node's SkyParams (a _lib.SkyParams); mark_dirty restarts its time-sliced g_skyCubemap bake (SkyNode::MarkDirty)"""
        return self.rt.sailor_rt_sky_set_params(self.h, C.byref(params), 1 if mark_dirty else 0)

    def sky_set_cloud_textures(self, weather, low, high) -> int:
        """publish the cloud march's textures to the Sky node (caller-owned uint8 device tensors: weather [h, w, 4], the noise volumes [n, n, n], x fastest);
        with them and cloudsDensity > 0 the node draws the clouds, the sun behind them and the clouds blit.  -1 if the graph has no Sky node"""
        assert weather.dim() == 3 and weather.shape[2] == 4 and low.dim() == 3 and high.dim() == 3 and len(set(low.shape)) == 1 and len(set(high.shape)) == 1
        for t in (weather, low, high):
            assert t.is_contiguous() and t.element_size() == 1, (t.dtype, tuple(t.shape))
        return self.rt.sailor_rt_sky_set_cloud_textures(self.h, weather.data_ptr(), weather.shape[1], weather.shape[0], low.data_ptr(), low.shape[0], high.data_ptr(),
                                                        high.shape[0])

    def sky_set_stars(self, vertices, count: int) -> int:
        """publish the star mesh to the Sky node: `vertices` = star_vertices(positions, colours) on the device, caller-owned.  With it and
        "Shaders/Stars.shader" enabled the node draws the star points.  -1 if the graph has no Sky node"""
        assert vertices.is_contiguous() and vertices.element_size() == 4 and vertices.numel() >= (count * 3 + 3) // 4 * 4 + count * 4, (vertices.dtype, vertices.numel())
        return self.rt.sailor_rt_sky_set_stars(self.h, vertices.data_ptr(), count)

    def set_particles(self, particles: int, frames: int, fps: int, trace_frames: int, trace_decay: float, records, vertices, indices, map_extent=(4096, 4096),
                      material_instance: int = 0) -> int:
        """publish what the ExperimentalParticles node's loaders would have loaded: the header fields, `records` (host, _lib.PARTICLE_DATA_DTYPE), the particle
        mesh on the device (72-byte vertices, uint32 indices; caller-owned) and the extent of the node's shadow map.  -1 if the graph has no such node"""
        import numpy as np
        records = np.ascontiguousarray(records)
        assert records.dtype.itemsize == 80 and vertices.is_contiguous() and indices.is_contiguous()
        num_vertices, num_indices = vertices.numel() * vertices.element_size() // 72, indices.numel() * indices.element_size() // 4
        return self.rt.sailor_rt_set_particles(self.h, particles, frames, fps, trace_frames, trace_decay, records.ctypes.data, len(records), vertices.data_ptr(),
                                               num_vertices, indices.data_ptr(), num_indices, material_instance, map_extent[0], map_extent[1])

    def particles_buffers(self):
        """(device pointer of the ExperimentalParticles node's instance SSBO, its instance count, device pointer of its shadow map, the map's width, height);
        the pointers are None before the node's first frame; raises if the graph has no such node"""
        inst, count, smap, w, h = C.c_void_p(), C.c_uint32(0), C.c_void_p(), C.c_int(0), C.c_int(0)
        if self.rt.sailor_rt_particles_buffers(self.h, C.byref(inst), C.byref(count), C.byref(smap), C.byref(w), C.byref(h)) != 0:
            raise ValueError("the graph has no ExperimentalParticles node")
        return inst.value, count.value, smap.value, w.value, h.value

    def sky_state(self):
        """(m_updateEnvCubemapPattern, m_bIsDirty) of the Sky node; raises if the graph has none"""
        pattern, dirty = C.c_int(0), C.c_int(0)
        if self.rt.sailor_rt_sky_state(self.h, C.byref(pattern), C.byref(dirty)) != 0:
            raise ValueError("the graph has no Sky node")
        return pattern.value, dirty.value

    def set_environment_map(self, equirect, repeat=True, irradiance_size=0):
        """hand the Environment node its "EnvironmentMap" panorama (float32 [H, W, 4] device tensor): it converts it to the raw 512 x 512 x 6 cube"""
        return self.rt.sailor_rt_set_environment_map(self.h, equirect.data_ptr(), equirect.shape[1], equirect.shape[0], 1 if repeat else 0, irradiance_size)

    def sampler(self, name: str):
        """(device pointer, width, height, mip levels) of a sampler published by the graph's nodes"""
        w, h, l = C.c_int(0), C.c_int(0), C.c_int(0)
        p = self.rt.sailor_rt_sampler(self.h, name.encode(), C.byref(w), C.byref(h), C.byref(l))
        return p, w.value, h.value, l.value

    def build_depth_highz(self, depth, width, height, levels):
        """run the DepthHighZ node over a float32 [h, w] device tensor; returns (status, device pointer of the level-major pyramid)"""
        p = C.c_void_p()
        st = self.rt.sailor_rt_build_depth_highz(self.h, depth.data_ptr() if depth is not None else None, depth.shape[1] if depth is not None else 0,
                                                 depth.shape[0] if depth is not None else 0, width, height, levels, C.byref(p))
        return st, p.value

    def ecs_sweep_traced(self, entities, trace: str = "octree", octree_root_size: int | None = None):
        """EcsSweepSystem (host arrays uploaded by the driver) with its trace mode set, ticked against the scene view's camera (set_camera):
        returns (status, device pointers of the world matrices, world boxes, visibility words, inserted words -- None in flat mode)"""
        mode = _lib.trace_mode(trace)
        trs = np.ascontiguousarray(entities.transforms, np.float32)
        par = np.ascontiguousarray(entities.parent, np.uint32)
        box = np.ascontiguousarray(entities.local_aabb, np.float32)
        offs = np.ascontiguousarray(entities.level_offsets, np.uint32)
        w, a, v, ins = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        st = self.rt.sailor_rt_ecs_sweep_traced(self.h, trs.ctypes.data, par.ctypes.data, box.ctypes.data, len(par), offs.ctypes.data, len(offs) - 1, mode,
                                                0 if octree_root_size is None else octree_root_size, C.byref(w), C.byref(a), C.byref(v), C.byref(ins))
        return st, w.value, a.value, v.value, ins.value

    def load_world(self, text: str, width: int, height: int, max_objects: int = 4096):
        """load a `.world`: camera -> scene view, LightComponents -> LightingECS (packed by Tick); returns (transforms float32 [n, 12], parents uint32 [n],
        number of lights, number of mesh renderers) for the ECS sweep"""
        import numpy as np
        tr = np.zeros((max_objects, 12), np.float32)
        par = np.zeros(max_objects, np.uint32)
        nl, nm = C.c_int(0), C.c_int(0)
        n = self.rt.sailor_rt_load_world(self.h, text.encode(), width, height, tr.ctypes.data, par.ctypes.data, max_objects, C.byref(nl), C.byref(nm))
        if n < 0:
            raise ValueError("the .world text does not parse")
        return tr[:n], par[:n], nl.value, nm.value

    def load_renderer(self, text: str):
        """FrameGraphImporter::BuildFrameGraph from a `.renderer` text: (nodes created, nodes without a class here, render targets created)"""
        skipped, targets = C.c_int(0), C.c_int(0)
        n = self.rt.sailor_rt_load_renderer(self.h, text.encode(), C.byref(skipped), C.byref(targets))
        if n < 0:
            raise ValueError("the .renderer text does not parse")
        return n, skipped.value, targets.value

    def render_target(self, name: str):
        w, h, l = C.c_int(0), C.c_int(0), C.c_int(0)
        p = self.rt.sailor_rt_render_target(self.h, name.encode(), C.byref(w), C.byref(h), C.byref(l))
        return p, w.value, h.value, l.value

    def set_render_target(self, name: str, tensor):
        """publish a float32 [h, w] device tensor as a named render target (DepthBuffer, ...)"""
        self.rt.sailor_rt_set_render_target(self.h, name.encode(), tensor.data_ptr(), tensor.shape[1], tensor.shape[0])

    def set_sampler(self, name: str, tensor, width: int, height: int) -> int:
        """publish a float32 [height, width, 4] device tensor of decoded linear texels under a sampler name of the `.renderer` text
        (g_noiseSampler: the file texture the parser records and does not load); the tensor must outlive the graph"""
        assert tuple(tensor.shape) == (height, width, 4) and tensor.is_contiguous(), tuple(tensor.shape)
        return self.rt.sailor_rt_set_sampler(self.h, name.encode(), tensor.data_ptr(), width, height)

    def set_color_target(self, name: str, tensor):
        """publish a float32 [h, w, 4] device tensor as a named RGBA render target (the HDR target RenderScene's radiance stands for, an LDR target)"""
        self.rt.sailor_rt_set_color_target(self.h, name.encode(), tensor.data_ptr(), tensor.shape[1], tensor.shape[0])

    def set_color_target_chain(self, name: str, chain, width: int, height: int, levels: int):
        """publish a flat float32 device tensor holding a level-major RGBA mip chain (host.mip_chain_texels(width, height, levels) * 4 floats) as a named
        render target with `levels` mip levels; its head is level 0 and may be the radiance tensor's storage"""
        from . import host
        assert chain.is_contiguous() and chain.numel() >= host.mip_chain_texels(width, height, levels) * 4, chain.numel()
        if self.rt.sailor_rt_set_color_target_chain(self.h, name.encode(), chain.data_ptr(), width, height, levels) != 0:
            raise ValueError(f"bad mip chain {width} x {height} x {levels}")

    def enable_node(self, name: str):
        """opt this runtime's graphs in to a node class that is compiled in but not registered ("Bloom"): load_renderer / build_graph then create it"""
        if self.rt.sailor_rt_enable_node(self.h, name.encode()) != 0:
            raise ValueError(f"no opt-in node class {name!r}")

    def enable_shader(self, path: str):
        """opt this runtime in to a shader that has an entry point but is not routed by default ("Shaders/MotionBlur.shader", "Shaders/Debug.shader":
        PostProcess entries loaded afterwards draw with it; "Shaders/Stars.shader", "Shaders/SunShafts.shader": the Sky node draws its star points and sun
        shafts, when enabled before the first frame)"""
        if self.rt.sailor_rt_enable_shader(self.h, path.encode()) != 0:
            raise ValueError(f"no opt-in shader {path!r}")

    def launch_log(self, max_names: int = 16):
        """(count, names): how many kernels the driver's context has launched, and the names of the last few, oldest first"""
        count = C.c_uint64()
        names = (C.c_char_p * max_names)()
        if self.rt.sailor_rt_launch_log(self.h, C.byref(count), names, max_names) != 0:
            raise ValueError("no launch log")
        return int(count.value), [n.decode() for n in names if n is not None]

    def set_time(self, delta_time: float, current_time: float = 0.0):
        """sceneView.m_deltaTime / m_currentTime of the frames processed from here on"""
        self.rt.sailor_rt_set_time(self.h, delta_time, current_time)

    def eye_adaptation_state(self):
        """(device pointer of the EyeAdaptation node's 256 histogram counts, device pointer of its adapted-luminance word); raises if the graph has no such node"""
        hist, lum = C.c_void_p(), C.c_void_p()
        if self.rt.sailor_rt_eye_adaptation_state(self.h, C.byref(hist), C.byref(lum)) != 0:
            raise ValueError("the graph has no EyeAdaptation node that has processed a frame")
        return hist.value, lum.value

    def shadow_pass(self, light_matrix, positions, indices, models, first_instance, instance_count, shadow_map, evsm, radius_umbra=0.0, radius_penumbra=0.0):
        """one shadow pass of ShadowPrepassNode (caster draw + fragment stage + blur) over device tensors; the map is float32 [S, S, 4] (EVSM) or float16 [S, S]"""
        lm = np.ascontiguousarray(light_matrix, np.float32).reshape(16)
        return self.rt.sailor_rt_shadow_pass(self.h, lm.ctypes.data_as(C.POINTER(C.c_float)), positions.data_ptr(), positions.shape[0], indices.data_ptr(),
                                             indices.numel(), models.data_ptr(), first_instance, instance_count, shadow_map.data_ptr(), shadow_map.shape[0],
                                             1 if evsm else 0, radius_umbra, radius_penumbra)

    def gpu_culling(self, instances, num_instances, first_instance, batches, num_batches):
        """the "GPU Culling" Dispatch of RHIRecordDrawCallGPUCulling over uint8 / int32 device tensors, in place"""
        return self.rt.sailor_rt_gpu_culling(self.h, instances.data_ptr(), num_instances, first_instance,
                                             batches.data_ptr() if batches is not None else None, num_batches)

    def set_surface(self, surface_tensor, radiance_tensor):
        self.rt.sailor_rt_set_surface(self.h, surface_tensor.data_ptr(), radiance_tensor.data_ptr(), surface_tensor.shape[2], surface_tensor.shape[1])

    def set_scene(self, vertices, indices, instances, materials, textures, num_textures: int, batches, texture_levels=None):
        """what RenderScene draws without a `surface` resource: device tensors of 72-byte vertices, int32 indices, 96-byte instances, 80-byte materials and
        the SailorTextureDesc table (any of the last three None = that binding missing), and batches uint32 [n, 5] = indexCount, instanceCount, firstIndex,
        vertexOffset, firstInstance.  texture_levels: RHITexture::GetMipLevels() of the table's textures, one int per descriptor (the host's knowledge of
        them): with an entry above 1 the pass takes the entry points with the implicit level of detail; None: the one-level route"""
        nbytes = lambda t: t.numel() * t.element_size()
        b = np.ascontiguousarray(batches, np.uint32).reshape(-1, 5)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.call("sailor_rt_set_scene", ptr(vertices), nbytes(vertices) // 72, ptr(indices), indices.numel(), ptr(instances),
                  0 if instances is None else nbytes(instances) // 96, ptr(materials), 0 if materials is None else nbytes(materials) // 80, ptr(textures), num_textures,
                  b.ctypes.data, len(b))
        if texture_levels is not None:
            levels = np.ascontiguousarray(texture_levels, np.uint32)
            self.call("sailor_rt_set_scene_texture_levels", levels.ctypes.data if len(levels) else None, len(levels))

    def generate_texture_mips(self, image, srgb: bool) -> np.ndarray:
        """IGraphicsDriver::CreateTexture with a full chain + GenerateMipMaps for one uint8 [H, W, 4] image -> the whole chain as uint32 texels, level after level"""
        from . import host
        img = np.ascontiguousarray(image, np.uint8)
        h, w = img.shape[:2]
        out = np.zeros(host.mip_chain_texels(w, h, host.texture_mip_levels(w, h)), np.uint32)
        self.call("sailor_rt_generate_texture_mips", img.ctypes.data, w, h, 1 if srgb else 0, out.ctypes.data, out.size)
        return out

    def set_scene_tags(self, tags, flags):
        """the materials of set_scene's batches, after set_scene: tags = one render queue tag per batch ("Opaque", "Masked", "" = untagged: drawn by every
        RenderScene node), flags = one int per batch, BATCH_ALPHA_CUTOUT | BATCH_DOUBLE_SIDED"""
        assert len(tags) == len(flags)
        f = np.ascontiguousarray(flags, np.uint32)
        self.call("sailor_rt_set_scene_tags", ",".join(tags).encode(), f.ctypes.data if len(f) else None, len(f))

    def set_scene_shaders(self, shaders):
        """the shaders of set_scene's batches, after set_scene: one int per batch, SHADER_STANDARD (Standard.shader) or SHADER_STANDARD_GLTF (Standard_glTF.shader,
        what an imported model's material uses: its slots of the material table are that shader's records)"""
        s = np.ascontiguousarray(shaders, np.uint32)
        self.call("sailor_rt_set_scene_shaders", s.ctypes.data if len(s) else None, len(s))

    def set_scene_blend(self, blend_modes, z_write):
        """the blend mode and the z-write of set_scene's batches' materials, after set_scene: one EBlendMode per batch (0 None, 1 Additive, 2 AlphaBlending,
        3 Multiply) and one 0 / 1.  A RenderScene pass whose batches all have z-write off is the Transparent queue's: peeled by primitive order and blended"""
        b, z = np.ascontiguousarray(blend_modes, np.uint32), np.ascontiguousarray(z_write, np.uint32)
        assert len(b) == len(z)
        self.call("sailor_rt_set_scene_blend", b.ctypes.data if len(b) else None, z.ctypes.data if len(z) else None, len(b))

    def set_transparent_layers(self, layers: int):
        """the layer budget of a transparent pass (default 4)"""
        self.call("sailor_rt_set_transparent_layers", layers)

    def set_transparent_mode(self, mode: int):
        """the route of a transparent pass: 0 = the peel (default), 1 = per-pixel fragment buckets (one rasterisation a pass, (budget + 1) x 8 bytes a pixel)"""
        self.call("sailor_rt_set_transparent_mode", mode)

    def transparent_overflow(self) -> int:
        """the pixels that still had a fragment behind the budget's layers in the last frame's transparent pass.  SYNCHRONISES with the stream: read it after the
        frame or at the next frame's start"""
        n = self.rt.sailor_rt_transparent_overflow(self.h)
        if n < 0:
            raise _lib.SailorHipError(-1, "sailor_rt_transparent_overflow")
        return int(n)

    def set_scene_targets(self, color, depth=None):
        """RenderScene's colour attachment (float32 [H, W, 4]) and the prepass's raw depth (float32 [H, W]) or None"""
        self.call("sailor_rt_set_scene_targets", color.data_ptr(), None if depth is None else depth.data_ptr(), color.shape[1], color.shape[0])

    def set_shadow_maps(self, map_tensors, formats, lights_matrices):
        ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in map_tensors])
        sizes = (C.c_int * 4)(*[t.shape[0] for t in map_tensors])
        fmts = (C.c_int * 4)(*formats)
        lm = np.ascontiguousarray(lights_matrices, np.float32).reshape(64)
        self.rt.sailor_rt_set_shadow_maps(self.h, ptrs, sizes, fmts, lm.ctypes.data)

    def set_caster_data(self, world_aabb, last_changed_frames, cast_shadows=None, resolutions=None, trace: str | None = None, octree_root_size: int | None = None):
        """The scene's caster data, after set_scene: world_aabb = float32 [n, 6] device tensor of the scene's instances' world boxes (the ECS sweep's output;
        it must outlive the runtime's use of it), last_changed_frames = one frame number per instance, cast_shadows = m_bCastShadows as uint64 words or None
        (every instance casts), resolutions = the four cascade maps' sizes or None (the reference's 4096), trace = "flat" | "octree" | None (as the runtime's
        sweep system traces).  From then on process_frame() plans the cascades first and a ShadowPrepass node draws them.  world_aabb None takes it away."""
        if world_aabb is None:
            self.call("sailor_rt_set_caster_data", None, 0, None, None, None, 0, 0)
            return
        n = world_aabb.shape[0]
        assert world_aabb.is_contiguous() and world_aabb.numel() * world_aabb.element_size() == 24 * n, tuple(world_aabb.shape)
        frames = np.ascontiguousarray(last_changed_frames, np.uint64)
        assert len(frames) == n
        cast = None if cast_shadows is None else np.ascontiguousarray(cast_shadows, np.uint64)
        assert cast is None or len(cast) == (n + 63) // 64
        res = None if resolutions is None else (C.c_int * 4)(*[int(r) for r in resolutions])
        mode = 0xFFFFFFFF if trace is None else _lib.trace_mode(trace)
        self.call("sailor_rt_set_caster_data", world_aabb.data_ptr(), n, None if cast is None else cast.ctypes.data, frames.ctypes.data, res, mode,
                  0 if octree_root_size is None else octree_root_size)

    def set_light_rotation(self, index: int, rotation):
        """the owner's rotation (x, y, z, w) of light `index`: with its position the transform whose inverse is the light's view matrix"""
        q = np.ascontiguousarray(rotation, np.float32).reshape(4)
        self.call("sailor_rt_set_light_rotation", index, q.ctypes.data)

    def shadow_passes(self, num_instances: int = 0):
        """sceneView.m_shadowMapsToUpdate of the last process_frame(): one dict per pass -- cascade (m_lighMatrixIndex), shadow_type, casters, dependencies
        (m_internalCommandsList) and, with num_instances, mask (the pass's caster set as uint64 words)"""
        words = (num_instances + 63) // 64
        info, masks = np.zeros((64, 8), np.uint32), np.zeros((64, max(words, 1)), np.uint64)
        n = self.rt.sailor_rt_shadow_passes(self.h, info.ctypes.data, masks.ctypes.data if words else None, words, 64)
        return [{"cascade": int(i[0]), "shadow_type": int(i[1]), "casters": int(i[2]), "dependencies": [int(d) for d in i[4:4 + int(i[3])]],
                 "mask": masks[p, :words].copy()} for p, i in enumerate(info[:max(n, 0)])]

    def csm_shadow_map(self, cascade: int):
        """(device pointer, size, SAILOR_SHADOWMAP_* format) of cascade map `cascade` of the runtime's LightingECS; pointer None before it exists"""
        size, fmt = C.c_int(0), C.c_int(0)
        p = self.rt.sailor_rt_csm_shadow_map(self.h, cascade, C.byref(size), C.byref(fmt))
        return p, size.value, fmt.value

    def lights_matrices(self) -> np.ndarray:
        """`lightsMatrices` of the lights set: float32 [4, 16]"""
        out = np.zeros((4, 16), np.float32)
        if self.rt.sailor_rt_lights_matrices(self.h, out.ctypes.data) != 0:
            raise ValueError("the lights set has no lightsMatrices")
        return out

    def set_frame_split(self, rank: int, world_size: int, comm=None):
        """this runtime renders tile-row band `rank` of `world_size`; per-pixel targets set afterwards hold the band's rows"""
        self.call("sailor_rt_set_frame_split", rank, world_size, C.c_void_p(comm) if comm else None)

    def exchange_light_lists(self, global_grid, global_culled):
        self.call("sailor_rt_exchange_light_lists", global_grid.data_ptr(), global_grid.numel() * global_grid.element_size(), global_culled.data_ptr(),
                  global_culled.numel() * global_culled.element_size())

    # ---- the world's DebugContext (RHI/DebugContext.cpp): what the DebugDraw node draws; `duration` is the line's lifetime in seconds of debug_tick ----
    @staticmethod
    def _fv(v, n):
        a = np.ascontiguousarray(v, np.float32).reshape(-1)
        assert a.size == n, (a.size, n)
        return a

    def debug_draw_line(self, start, end, color, duration: float = 0.0):
        a, b, c = self._fv(start, 3), self._fv(end, 3), self._fv(color, 4)
        assert self.rt.sailor_rt_debug_draw_line(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data, duration) == 0

    def debug_draw_aabb(self, aabb_min, aabb_max, color, duration: float = 0.0):
        a, b, c = self._fv(aabb_min, 3), self._fv(aabb_max, 3), self._fv(color, 4)
        assert self.rt.sailor_rt_debug_draw_aabb(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data, duration) == 0

    def debug_draw_arrow(self, start, end, color, duration: float = 0.0):
        a, b, c = self._fv(start, 3), self._fv(end, 3), self._fv(color, 4)
        assert self.rt.sailor_rt_debug_draw_arrow(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data, duration) == 0

    def debug_draw_frustum(self, corners, color, duration: float = 0.0):
        """corners: Frustum::GetCorners(), 8 x 3 (host.extract_frustum_planes' second result)"""
        a, c = self._fv(corners, 24), self._fv(color, 4)
        assert self.rt.sailor_rt_debug_draw_frustum(self.h, a.ctypes.data, c.ctypes.data, duration) == 0

    def debug_draw_origin(self, position, origin, size: float = 1.0, duration: float = 0.0):
        a, m = self._fv(position, 3), self._fv(origin, 16)
        assert self.rt.sailor_rt_debug_draw_origin(self.h, a.ctypes.data, m.ctypes.data, size, duration) == 0

    def debug_draw_sphere(self, position, radius: float, color, duration: float = 0.0):
        a, c = self._fv(position, 3), self._fv(color, 4)
        assert self.rt.sailor_rt_debug_draw_sphere(self.h, a.ctypes.data, radius, c.ctypes.data, duration) == 0

    def debug_tick(self, delta_time: float) -> int:
        """DebugContext::Tick: upload the line list, then run the lifetimes down by delta_time (a line below zero leaves AFTER the frame of this tick);
        returns the number of vertices the next frame draws"""
        return self.rt.sailor_rt_debug_tick(self.h, delta_time)

    def debug_vertices(self) -> np.ndarray:
        """the line list as it stands: VertexP3C4 records (_lib.VERTEX_P3C4_DTYPE), two per line"""
        n = self.rt.sailor_rt_debug_vertices(self.h, None, 0)
        out = np.zeros(max(n, 0), _lib.VERTEX_P3C4_DTYPE)
        if n > 0:
            self.rt.sailor_rt_debug_vertices(self.h, out.ctypes.data, n)
        return out

    def set_ui_draw_data(self, draw_data: dict | None, font: np.ndarray | None = None) -> int:
        """The frame's ImGui draw data (sailor_amd.host.ui_draw_data: display_pos, display_size, framebuffer_scale, lists of vertices, indices and cmds), which
        the RenderImGui node draws over its colour attachment; None takes it away.  font: the atlas, uint8 [h, w, 4] (R8G8B8A8_UNORM), bound as `sTexture`
        from this call on.  Indices are 16-bit, as ImDrawIdx is.  Returns the number of commands that will draw."""
        lists = draw_data.get("lists", []) if draw_data else []
        if not lists or sum(len(l["vertices"]) for l in lists) == 0:
            assert self.rt.sailor_rt_set_ui_draw_data(self.h, None, None, None, None, 0, None, 0, None, 0, None, 0, None, 0, 0) == 0
            return 0
        flat = [c for l in lists for c in l["cmds"]]
        cl, cc, first = (_lib.UiDrawList * len(lists))(), (_lib.UiDrawCmd * max(len(flat), 1))(), 0
        for n, l in enumerate(lists):
            cl[n] = _lib.UiDrawList(len(l["vertices"]), len(l["indices"]), first, len(l["cmds"]))
            first += len(l["cmds"])
        for n, c in enumerate(flat):
            cc[n] = _lib.UiDrawCmd((C.c_float * 4)(*[float(x) for x in c["clip_rect"]]), int(c.get("elem_count", 0)), int(c.get("idx_offset", 0)),
                                   int(c.get("vtx_offset", 0)), int(c.get("callback", _lib.UI_CALLBACK_NONE)))
        v = np.ascontiguousarray(np.concatenate([np.asarray(l["vertices"], _lib.VERTEX_P2UV2C1_DTYPE) for l in lists]))
        i = np.concatenate([np.asarray(l["indices"], np.uint32) for l in lists])
        assert len(i) and int(i.max()) < 65536, "ImDrawIdx is 16 bits"
        i = np.ascontiguousarray(i.astype(np.uint16))
        pos, size, fbs = (np.ascontiguousarray(draw_data[k], np.float32) for k in ("display_pos", "display_size", "framebuffer_scale"))
        f = None if font is None else np.ascontiguousarray(font, np.uint8)
        assert f is None or (f.ndim == 3 and f.shape[2] == 4)
        n = self.rt.sailor_rt_set_ui_draw_data(self.h, pos.ctypes.data, size.ctypes.data, fbs.ctypes.data, v.ctypes.data, len(v), i.ctypes.data, len(i), cl, len(lists), cc,
                                               len(flat), None if f is None else f.ctypes.data, 0 if f is None else f.shape[1], 0 if f is None else f.shape[0])
        if n < 0:
            raise _lib.SailorHipError(-1, "sailor_rt_set_ui_draw_data")
        return n

    def node_indirect_commands(self, node_index: int, max_commands: int = 64) -> np.ndarray:
        """the indirect buffer of node `node_index` of the graph (a DepthPrepass node, a RenderScene node under `GPUCulling: true`) after its last frame,
        downloaded: uint32 [commands, 5] = (indexCount, instanceCount, firstIndex, vertexOffset, firstInstance)"""
        out = np.zeros((max_commands, 5), np.uint32)
        n = self.rt.sailor_rt_node_indirect_commands(self.h, node_index, out.ctypes.data, max_commands)
        if n < 0:
            raise ValueError(f"node {node_index} owns no indirect buffer")
        return out[:min(n, max_commands)]

    def last_frame_regions(self):
        """the debug regions of the last process_frame in the order the driver executed their BeginDebugRegion commands while it submitted the frame's lists"""
        buf = C.create_string_buffer(1 << 14)
        n = self.rt.sailor_rt_last_frame_regions(self.h, buf, len(buf))
        return buf.value.decode().split(";") if n > 0 else []

    def draw_indexed_indirect(self, shader_path: str, depth) -> int:
        """one depth-only pass of one DrawIndexedIndirect over the scene's batch 0 with a material of that shader, submitted at once -> the driver's status"""
        return self.rt.sailor_rt_draw_indexed_indirect(self.h, shader_path.encode(), depth.data_ptr(), depth.shape[1], depth.shape[0])

    def process_frame(self) -> int:
        return self.rt.sailor_rt_process_frame(self.h)

    def capture_next_frame(self, capacities: dict, storage) -> int:
        """Arm a capture of the next process_frame() (a test facility; off unless armed): `capacities` maps resource names -- a render target or published
        sampler / cube of the graph, "lightsGrid", "culledLights", "light", "lightsMatrices", "csm0" .. "csm3", "eyeAdaptation", "indirect<node index>" -- to the
        bytes reserved for each; `storage` is a contiguous uint8 device tensor of at least (nodes + 2) * sum(capacities) bytes that must outlive the frame.
        Slot 0 is taken before the frame's transfer list, slot 1 before the first entry (after the whole transfer list), slot 2 + i after entry i.  Returns the
        number of slots; raises while the stream is being captured into a hipGraph.  Read the frame with captured_frame() after wait_idle()."""
        names = list(capacities)
        assert names and all("," not in n for n in names) and storage.is_contiguous() and storage.element_size() == 1
        caps = (C.c_size_t * len(names))(*[int(capacities[n]) for n in names])
        slots = self.rt.sailor_rt_capture_next_frame(self.h, ",".join(names).encode(), caps, len(names), storage.data_ptr(), storage.numel())
        if slots < 0:
            raise _lib.SailorHipError(slots, "sailor_rt_capture_next_frame")
        self._capture = (names, [int(capacities[n]) for n in names], storage, slots)
        return slots

    def captured_frame(self):
        """the armed frame, after wait_idle(): one dict per slot, name -> uint8 device tensor (a view of the storage, as long as the resource was at that slot);
        a resource absent at a slot is left out"""
        names, caps, storage, slots = self._capture
        table = np.full(slots * len(names), -1, np.int64)
        n = self.rt.sailor_rt_capture_result(self.h, table.ctypes.data, table.size)
        assert n == table.size, (n, table.size)
        table = table.reshape(slots, len(names))
        too_large = [names[k] for k in range(len(names)) if (table[:, k] == -2).any()]
        if too_large:
            raise ValueError(f"larger than the capacity given for them: {too_large}")
        stride, out = sum(caps), []
        for s in range(slots):
            at, row = s * stride, {}
            for k, name in enumerate(names):
                if table[s, k] >= 0:
                    row[name] = storage[at:at + int(table[s, k])]
                at += caps[k]
            out.append(row)
        return out

    def process_frame_overwriting_lists(self, grid, culled) -> int:
        """one frame with an UpdateBuffer of lightsGrid / culledLights (numpy uint32 arrays or None) recorded between the LightCulling node and RenderScene"""
        import numpy as np
        g = None if grid is None else np.ascontiguousarray(grid, np.uint32)
        c = None if culled is None else np.ascontiguousarray(culled, np.uint32)
        return self.rt.sailor_rt_process_frame_overwriting_lists(self.h, None if g is None else g.ctypes.data, 0 if g is None else g.nbytes,
                                                                 None if c is None else c.ctypes.data, 0 if c is None else c.nbytes)

    def wait_idle(self):
        self.rt.sailor_rt_wait_idle(self.h)

    def buffer(self, name: str):
        n = C.c_size_t(0)
        p = self.rt.sailor_rt_buffer(self.h, name.encode(), C.byref(n))
        return p, n.value


def star_vertices(positions, colors):
    """the star mesh as the Sky node's vertex buffer: the VertexP3C4 mesh de-interleaved -- count x 3 floats of positions, then, at the next 16-byte
    boundary, count x 4 floats of colours -> float32 [n]"""
    import numpy as np
    positions, colors = np.ascontiguousarray(positions, np.float32).reshape(-1, 3), np.ascontiguousarray(colors, np.float32).reshape(-1, 4)
    count = positions.shape[0]
    assert colors.shape[0] == count
    out = np.zeros((count * 3 + 3) // 4 * 4 + count * 4, np.float32)
    out[:count * 3] = positions.reshape(-1)
    out[(count * 3 + 3) // 4 * 4:] = colors.reshape(-1)
    return out
