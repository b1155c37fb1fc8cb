"""Torch-facing handle on the HIP Forward+ path: device memory and streams come from torch, every kernel comes from
libsailor_hip.so through the C-ABI (include/sailor_hip.h).  One object = one GPU = one band of the frame.

Mirrors the two reference passes that own these buffers:
  * LightCullingNode (FrameGraph/LightCullingNode.cpp:59-77): owns `culledLights` / `lightsGrid`, dispatches the cull;
  * RenderSceneNode + Standard.shader (FrameGraph/RenderSceneNode.cpp:109): consumes them while shading.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib, host
from ._lib import Band, CsmDesc, UboFrameData

LIGHTS_PER_TILE = _lib.LIGHTS_PER_TILE


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _ref(s):
    """a structure by reference, or NULL"""
    return None if s is None else C.byref(s)


class HipContext:
    """RAII wrapper of SailorHipContext bound to a torch device and stream."""

    def __init__(self, device: torch.device | str | int = "cuda:0", stream: torch.cuda.Stream | None = None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SailorHipError(-2, "HipContext", "a HIP device is required (there is no CPU fallback)")
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        handle = C.c_void_p()
        _lib.call("sailor_hip_context_create", index, C.c_void_p(self.stream.cuda_stream), 0, C.byref(handle))
        self.handle = handle
        self._lib = _lib.load()

    def call(self, name: str, *args):
        """the checked call of the C-ABI entry `name`, which takes this context first: a status other than 0 raises under the entry's name, with the context's
        last error"""
        _lib.check(getattr(self._lib, name)(self.handle, *args), name, self.handle)

    def synchronize(self):
        self.call("sailor_hip_context_synchronize")

    def time_launches(self, first_slot: int, count: int):
        """the next `count` kernel launches through this context carry event pairs on their dispatch packets (sailor_hip_context_time_launches)"""
        self.call("sailor_hip_context_time_launches", first_slot, count)

    def timed_launch_ms(self, slot: int) -> float:
        ms = C.c_float()
        self.call("sailor_hip_context_timed_launch_ms", slot, C.byref(ms))
        return float(ms.value)

    def launch_log(self, max_names: int = 16):
        """(count, names): how many kernels the path's entry points have launched through this context, and the names of the last few, oldest first
        (sailor_hip_context_launch_log).  The kernels of ONE call = the names behind the count read in front of it."""
        count = C.c_uint64()
        names = (C.c_char_p * max_names)()
        self.call("sailor_hip_context_launch_log", C.byref(count), names, max_names)
        return int(count.value), [n.decode() for n in names if n is not None]

    def launches_of(self, fn):
        """the names of the kernels fn() launches through this context (at most 16)"""
        before, _ = self.launch_log(0)
        fn()
        after, names = self.launch_log(16)
        n = after - before
        assert n <= 16, n
        return names[len(names) - n:] if n else []

    def close(self):
        if getattr(self, "handle", None):
            self._lib.sailor_hip_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def linearize_depth(ctx: "HipContext", frame: UboFrameData, raw: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """LinearizeDepthNode (FrameGraph/LinearizeDepthNode.cpp:22): raw reversed-Z depth rows -> positive view distance."""
    assert raw.dtype == torch.float32 and raw.dim() == 2 and raw.is_contiguous()
    if out is None:
        out = torch.empty_like(raw)
    ctx.call("sailor_hip_linearize_depth", C.byref(frame), _ptr(raw), _ptr(out), raw.shape[1], raw.shape[0])
    return out


_ENV_CULL_FLAGS = int(os.environ.get("SAILOR_CULL_FLAGS", "0"))


class PreparedLights:
    """sailor_hip_prepare_lights' output for a `light` SSBO of `capacity` records: the cull's 20-byte view and the shade's staged records, derived where
    the records are uploaded (the HIP backend does it behind UpdateShaderBinding) instead of in every frame's kernels.  prepare(first, count) after
    every change of the records [first, first + count)."""

    def __init__(self, ctx: "HipContext", lights: torch.Tensor, lights_num: int, capacity: int | None = None):
        self.ctx, self.lights, self.capacity = ctx, lights, max(int(capacity if capacity is not None else lights_num), 1)
        n = ctx._lib.sailor_hip_prepared_lights_size(self.capacity)
        self.buffer = torch.empty(n, dtype=torch.uint8, device=ctx.device)
        self.prepare(0, lights_num)

    def prepare(self, first: int, count: int, ctx: "HipContext | None" = None):
        (ctx or self.ctx).call("sailor_hip_prepare_lights", _ptr(self.lights), first, count, self.capacity, _ptr(self.buffer), self.buffer.numel())

    def views(self):
        """(posRadius float32 [capacity, 4], type int32 [capacity], staged float32 [capacity, 5, 4]) as tensors over the buffer"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.call("sailor_hip_prepared_lights_views", self.capacity, _ptr(self.buffer), C.byref(a), C.byref(b), C.byref(c))
        base = self.buffer.data_ptr()
        n = self.capacity
        f = self.buffer
        return (f[a.value - base: a.value - base + 16 * n].view(torch.float32).view(n, 4), f[b.value - base: b.value - base + 4 * n].view(torch.int32),
                f[c.value - base: c.value - base + 80 * n].view(torch.float32).view(n, 5, 4))


def _prepared_args(prepared: "PreparedLights | None", lights_num: int):
    """(the prepared buffer, its capacity) as the `_prepared` and `_tile_lists` entries take them: (NULL, 0) without prepared lights"""
    if prepared is None:
        return None, 0
    assert lights_num <= prepared.capacity
    return _ptr(prepared.buffer), prepared.capacity


class ForwardPlus:
    """Cull + shade for one band of a W x H frame on one GPU."""

    def __init__(self, ctx: HipContext, width: int, height: int, max_lights: int, band: Band | None = None, prepared: "PreparedLights | None" = None):
        """prepared: the prepared views of the light buffer this object will be used with -- cull() and shade() then hand them to the kernels unless told
        otherwise per call"""
        self.ctx, self.W, self.H, self.max_lights = ctx, width, height, max_lights
        self.prepared = prepared
        self.Tx, self.Ty = host.num_tiles(width, height)
        self.band = band if band is not None else host.band_whole_frame(width, height)
        self.band_tiles = (self.band.tileRowEnd - self.band.tileRowBegin) * self.Tx
        lib = ctx._lib
        ws = lib.sailor_hip_light_cull_workspace_size(width, height, max_lights, C.byref(self.band))
        if ws == 0:
            raise _lib.SailorHipError(-1, "light_cull_workspace_size")
        dev = ctx.device
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
        # LightCullingNode.cpp:64-65 (+1: the reference's buffer is one uint short when every tile is full)
        self.grid = torch.zeros(max(self.band_tiles, 1) * 2, dtype=torch.int32, device=dev)
        self.culled = torch.zeros(1 + max(self.band_tiles, 1) * LIGHTS_PER_TILE, dtype=torch.int32, device=dev)
        self.radiance = None
        # the cull's shading-order hint (long lists first) lives in the workspace; None = raster order
        self.tile_order = lib.sailor_hip_light_cull_tile_order(width, height, max_lights, C.byref(self.band), _ptr(self.workspace))
        self.use_tile_order = os.environ.get("SAILOR_NO_TILE_ORDER") is None
        self._culled_once = False
        # the cull's own per-tile form of the lists (tileNum[t] entries at tileLists[128 t ..]): what the shade reads by default -- the canonical
        # grid / culledLights are then only needed by other consumers, and k1_pack can run beside the shade (cull(..., defer_pack=True) + pack())
        a, b = C.c_void_p(), C.c_void_p()
        _lib.call("sailor_hip_light_cull_tile_lists", width, height, max_lights, C.byref(self.band), _ptr(self.workspace), C.byref(a), C.byref(b))
        self.tile_num, self.tile_lists = a.value, b.value
        self.shade_from_tile_lists = os.environ.get("SAILOR_SHADE_CANONICAL_LISTS") is None

    # -- K0 + K1 --------------------------------------------------------------------------------------------------
    def cull(self, frame: UboFrameData, lights: torch.Tensor, lights_num: int, depth: torch.Tensor, flags: int = _lib.CULL_DEFAULT,
             ctx: "HipContext | None" = None, prepared: "PreparedLights | None" = None, defer_pack: bool = False, prepare_lights: bool = False):
        """lights: uint8/any tensor holding lights_num 112-byte records; depth: float32 [band rows, W].
        ctx: record on another context's stream (frames in flight: next frame's cull beside this frame's shade).
        prepared: the lights' prepared views (the kernel then streams 20 bytes per light instead of the 112-byte records)."""
        assert depth.dtype == torch.float32 and depth.is_contiguous() and depth.shape == (self.band.fbRowCount, self.W), depth.shape
        assert lights_num <= self.max_lights
        prepared = prepared if prepared is not None else self.prepared
        flags |= _ENV_CULL_FLAGS   # (diagnostics)
        if defer_pack:             # the canonical buffers are written by pack(), wherever the caller records it
            flags |= _lib.CULL_DEFER_PACK
        if prepare_lights:         # every light dirty: the prepared views of all lights_num lights are (re)derived inside this cull
            assert prepared is not None
            flags |= _lib.CULL_PREPARE_LIGHTS
        pc = host.push_constants(frame, self.W, self.H, lights_num)
        (ctx or self.ctx).call("sailor_hip_light_cull_prepared", C.byref(frame), C.byref(pc), _ptr(lights), _ptr(depth), _ptr(self.grid), _ptr(self.culled),
                               self.culled.numel(), _ptr(self.workspace), self.workspace.numel(), C.byref(self.band), flags, *_prepared_args(prepared, lights_num))
        self._culled_once = True
        return self.grid, self.culled

    def pack(self, ctx: "HipContext | None" = None):
        """the second half of a cull(..., defer_pack=True): lightsGrid / culledLights from the per-tile lists, on ctx's stream (default: the cull's)"""
        (ctx or self.ctx).call("sailor_hip_light_cull_pack", self.W, self.H, self.max_lights, C.byref(self.band), _ptr(self.workspace), _ptr(self.grid),
                               _ptr(self.culled), self.culled.numel())

    # -- K2 + K3 --------------------------------------------------------------------------------------------------
    def shade(self, frame: UboFrameData, surface: torch.Tensor, lights: torch.Tensor, lights_num: int, csm: CsmDesc | None = None,
              out: torch.Tensor | None = None, ibl: "_lib.IblDesc | None" = None, prepared: "PreparedLights | None" = None,
              ctx: "HipContext | None" = None) -> torch.Tensor:
        """surface: float32 [3, band rows, W, 4]; returns radiance float32 [band rows, W, 4].  ibl: ambient term (its `ao`
        pointer, if any, holds the band's rows).  ctx: record on another context's stream."""
        ctx = ctx or self.ctx
        rows = self.band.fbRowCount
        assert surface.dtype == torch.float32 and surface.is_contiguous() and surface.shape == (3, rows, self.W, 4), surface.shape
        if out is None:
            if self.radiance is None:
                self.radiance = torch.empty((rows, self.W, 4), dtype=torch.float32, device=ctx.device)
            out = self.radiance
        prepared = prepared if prepared is not None else self.prepared
        order = self.tile_order if (self.use_tile_order and self._culled_once) else None  # only lists made by THIS object's cull have an order
        if self.shade_from_tile_lists and self._culled_once:
            # the lists where the cull left them (the same entries in the same order as grid / culledLights: the same radiance bit for bit)
            entry, lists = "sailor_hip_shade_tile_lists", (self.tile_num, self.tile_lists)
        else:
            entry, lists = "sailor_hip_shade_prepared", (_ptr(self.grid), _ptr(self.culled))
        ctx.call(entry, C.byref(frame), _ptr(surface), rows * self.W, _ptr(lights), lights_num, *lists, _ref(csm), _ref(ibl), _ptr(out), C.byref(self.band), order,
                 *_prepared_args(prepared, lights_num))
        return out

    # -- helpers ----------------------------------------------------------------------------------------------------
    def cull_diagnostics(self, lights_num: int) -> dict:
        out = (C.c_uint64 * 8)()
        self.ctx.call("sailor_hip_light_cull_diagnostics", self.W, self.H, lights_num, C.byref(self.band), _ptr(self.workspace), out)
        keys = ["bands", "mask_bits", "groups", "group_list_sum", "groups_overflowed", "group_list_max", "words_per_band", "column_mask_bits"]
        return dict(zip(keys, [int(v) for v in out]))

    def band_selection(self, lights_num: int):
        """(M, lightMap uint32[M]) of the last cull with lights_num lights, if that cull ran the band selection (the caller knows: HipContext.launches_of)"""
        a, b = C.c_void_p(), C.c_void_p()
        _lib.call("sailor_hip_light_cull_band_selection", self.W, self.H, lights_num, C.byref(self.band), _ptr(self.workspace), C.byref(a), C.byref(b))
        self.ctx.synchronize()
        base = self.workspace.data_ptr()
        m = int(self.workspace[a.value - base: a.value - base + 4].view(torch.int32).cpu().numpy().view(np.uint32)[0])
        lm = self.workspace[b.value - base: b.value - base + 4 * m].view(torch.int32).cpu().numpy().view(np.uint32).copy()
        return m, lm

    def lists_to_host(self):
        """(grid uint32[T,2], indices uint32[1 + total]) of this band, band-local offsets."""
        self.ctx.synchronize()
        g = self.grid.cpu().numpy().view(np.uint32).reshape(-1, 2)[: self.band_tiles]
        c = self.culled.cpu().numpy().view(np.uint32)
        return g.copy(), c[: 1 + int(c[0])].copy()


def upload_lights(lights: np.ndarray, device) -> torch.Tensor:
    assert lights.dtype.itemsize == 112
    raw = np.ascontiguousarray(lights).view(np.uint8).reshape(-1)
    if raw.size == 0:
        raw = np.zeros(112, np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


def upload_shadow_maps(shadows, device) -> tuple[CsmDesc, list]:
    """-> (CsmDesc with device pointers, tensors to keep alive).  A map that is None is passed as a null pointer: no map bound, shadow factor 1."""
    keep, maps = [], []
    for m in shadows.maps:
        if m is None:
            maps.append((0, 0, 0, _lib.SHADOWMAP_R16F))
            continue
        t = torch.from_numpy(np.ascontiguousarray(m)).to(device)
        keep.append(t)
        fmt = _lib.SHADOWMAP_R16F if m.dtype == np.float16 else (_lib.SHADOWMAP_RGBA32F if m.ndim == 3 else _lib.SHADOWMAP_R32F)
        maps.append((t.data_ptr(), m.shape[1], m.shape[0], fmt))
    return host.make_csm_desc(shadows.lights_matrices, maps), keep


def upload_ibl(ibl_set, device, ao_rows: tuple[int, int] | None = None) -> tuple["_lib.IblDesc", list]:
    """synth.IblSet -> (IblDesc with device pointers, tensors to keep alive); ao_rows = framebuffer rows of the band."""
    irr = torch.from_numpy(np.ascontiguousarray(ibl_set.irradiance)).to(device)
    env = torch.from_numpy(np.ascontiguousarray(ibl_set.env_chain)).to(device)
    lut = torch.from_numpy(np.ascontiguousarray(ibl_set.brdf_lut)).to(device)
    keep = [irr, env, lut]
    d = _lib.IblDesc()
    d.irradiance, d.irrSize = irr.data_ptr(), ibl_set.irradiance.shape[1]
    d.env, d.envSize, d.envLevels = env.data_ptr(), ibl_set.env_size, ibl_set.env_levels
    d.brdfLut, d.lutW, d.lutH = lut.data_ptr(), ibl_set.brdf_lut.shape[1], ibl_set.brdf_lut.shape[0]
    if ibl_set.ao is not None:
        a = ibl_set.ao if ao_rows is None else ibl_set.ao[ao_rows[0]:ao_rows[1]]
        ao = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        keep.append(ao)
        d.ao = ao.data_ptr()
    return d, keep


def evsm_blur(ctx: "HipContext", moments: torch.Tensor, radius_umbra: int, radius_penumbra: int, temp: torch.Tensor | None = None) -> torch.Tensor:
    """ShadowPrepassNode's blur of the cascade-0 EVSM map, in place; moments float32 [H, W, 4]."""
    assert moments.dtype == torch.float32 and moments.dim() == 3 and moments.shape[2] == 4 and moments.is_contiguous()
    if temp is None:
        temp = torch.empty_like(moments)
    ctx.call("sailor_hip_evsm_blur", _ptr(moments), _ptr(temp), moments.shape[1], moments.shape[0], radius_umbra, radius_penumbra)
    return moments


def evsm_blur_pass(ctx: "HipContext", src: torch.Tensor, radius_umbra: int, radius_penumbra: int, vertical: bool, out: torch.Tensor | None = None) -> torch.Tensor:
    """one pass of the blur ("Blur Horizontal" or "Blur Vertical") from src into another tensor; src float32 [H, W, 4]"""
    assert src.dtype == torch.float32 and src.dim() == 3 and src.shape[2] == 4 and src.is_contiguous()
    if out is None:
        out = torch.empty_like(src)
    ctx.call("sailor_hip_evsm_blur_pass", _ptr(src), _ptr(out), src.shape[1], src.shape[0], radius_umbra, radius_penumbra, int(vertical))
    return out


def compute_brdf_lut(ctx: "HipContext", width: int, height: int) -> torch.Tensor:
    """ComputeBrdfLut.shader on the GPU -> float32 [height, width, 2]"""
    out = torch.empty((height, width, 2), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_compute_brdf_lut", _ptr(out), width, height)
    return out


def compute_irradiance_map(ctx: "HipContext", env_chain: torch.Tensor, env_size: int, env_levels: int, size: int) -> torch.Tensor:
    """ComputeIrradianceMap.shader on the GPU: flat RGBA32F cube mip chain -> float32 [6, size, size, 4]"""
    out = torch.empty((6, size, size, 4), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_compute_irradiance_map", _ptr(env_chain), env_size, env_levels, _ptr(out), size)
    return out


def prefilter_env_map(ctx: "HipContext", raw_chain: torch.Tensor, size: int, levels: int) -> torch.Tensor:
    """EnvironmentNode's specular pre-filter (ComputeEnvMap_IBL.shader per mip) on the GPU: flat chain -> flat chain"""
    out = torch.empty_like(raw_chain)
    ctx.call("sailor_hip_prefilter_env_map", _ptr(raw_chain), _ptr(out), size, levels)
    return out


def cube_chain_floats(size: int, levels: int) -> int:
    """float count of the level-major RGBA32F cube chain (sailor_hip_generate_mipmaps_cube)"""
    return sum(6 * max(size >> l, 1) ** 2 * 4 for l in range(levels))


def raw_env_cubemap(ctx: "HipContext", equirect: torch.Tensor, size: int, levels: int, repeat: bool = True, cover=None) -> torch.Tensor:
    """EnvironmentNode.cpp:116-140: ConvertEquirect2Cubemap + GenerateMipMaps -> the flat RGBA32F chain of `rawEnvCubemap`.
    `equirect` is float32 [H, W, 4]; `cover` = (w, h) mirrors the reference's equirectExtent / 32 dispatch (default: the whole cube)."""
    assert equirect.dtype == torch.float32 and equirect.dim() == 3 and equirect.shape[2] == 4 and equirect.is_contiguous()
    chain = torch.zeros(cube_chain_floats(size, levels), dtype=torch.float32, device=ctx.device)
    cw, ch = (size, size) if cover is None else cover
    ctx.call("sailor_hip_equirect_to_cube", _ptr(equirect), equirect.shape[1], equirect.shape[0], 1 if repeat else 0, _ptr(chain), size, cw, ch)
    ctx.call("sailor_hip_generate_mipmaps_cube", _ptr(chain), size, levels)
    return chain


def sky_fill(ctx: "HipContext", frame: UboFrameData, params, width: int = _lib.SKY_RESOLUTION, height: int | None = None) -> torch.Tensor:
    """Sky.shader {FILL} (SkyNode.cpp:536-563): the atmosphere as seen through `frame` -> float32 [height, width, 4]"""
    height = width if height is None else height
    out = torch.empty((height, width, 4), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_sky_fill", C.byref(frame), C.byref(params), _ptr(out), width, height)
    return out


def sky_sun(ctx: "HipContext", frame: UboFrameData, params, size: int = _lib.SKY_SUN_RESOLUTION, clouds: torch.Tensor | None = None) -> torch.Tensor:
    """Sky.shader {SUN} (SkyNode.cpp:611-642): the sun disk -> float32 [size, size, 4]; `clouds` = None is the cleared clouds target"""
    out = torch.empty((size, size, 4), dtype=torch.float32, device=ctx.device)
    cw, ch = (0, 0) if clouds is None else (clouds.shape[1], clouds.shape[0])
    ctx.call("sailor_hip_sky_sun", C.byref(frame), C.byref(params), _ptr(clouds), cw, ch, _ptr(out), size, size)
    return out


def sky_compose(ctx: "HipContext", frame: UboFrameData, params, sky: torch.Tensor, sun: torch.Tensor, width: int, height: int,
                band: Band | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Sky.shader {COMPOSE} (SkyNode.cpp:644-680) over the rows of `band` (default: the whole frame) -> float32 [band rows, width, 4]"""
    for t in (sky, sun):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 4, (t.dtype, tuple(t.shape))
    band = band or host.band_whole_frame(width, height)
    if out is None:
        out = torch.empty((band.fbRowCount, width, 4), dtype=torch.float32, device=ctx.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (band.fbRowCount, width, 4), tuple(out.shape)
    ctx.call("sailor_hip_sky_compose", C.byref(frame), C.byref(params), _ptr(sky), sky.shape[1], sky.shape[0], _ptr(sun), sun.shape[1], sun.shape[0], _ptr(out), width,
             height, C.byref(band))
    return out


def sky_clouds(ctx: "HipContext", frame: UboFrameData, params, sky: torch.Tensor, weather: torch.Tensor, noise_low: torch.Tensor, noise_high: torch.Tensor,
               noise: torch.Tensor, linear_depth: torch.Tensor, width: int, height: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """Sky.shader {CLOUDS} (SkyNode.cpp:565-603): the cloud march -> float32 [height, width, 4], alpha = 1 - transmittance, row height - 1 = the top of
    the view.  weather: uint8 [h, w, 4]; noise_low / noise_high: uint8 [n, n, n] (z, y, x); noise: float32 [h, w, 4]; linear_depth: float32 [h, w]"""
    for t, dt, dims in ((sky, torch.float32, 3), (weather, torch.uint8, 3), (noise_low, torch.uint8, 3), (noise_high, torch.uint8, 3), (noise, torch.float32, 3),
                        (linear_depth, torch.float32, 2)):
        assert t.dtype == dt and t.is_contiguous() and t.dim() == dims, (t.dtype, tuple(t.shape))
    assert sky.shape[2] == 4 and weather.shape[2] == 4 and noise.shape[2] == 4
    assert len(set(noise_low.shape)) == 1 and len(set(noise_high.shape)) == 1, "the noise volumes are cubes"
    if out is None:
        out = torch.empty((height, width, 4), dtype=torch.float32, device=ctx.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (height, width, 4), tuple(out.shape)
    ctx.call("sailor_hip_sky_clouds", C.byref(frame), C.byref(params), _ptr(sky), sky.shape[1], sky.shape[0], _ptr(weather), weather.shape[1], weather.shape[0],
             _ptr(noise_low), noise_low.shape[0], _ptr(noise_high), noise_high.shape[0], _ptr(noise), noise.shape[1], noise.shape[0], _ptr(linear_depth),
             linear_depth.shape[1], linear_depth.shape[0], _ptr(out), width, height)
    return out


def sky_sun_clouds(ctx: "HipContext", frame: UboFrameData, params, clouds: torch.Tensor, size: int = _lib.SKY_SUN_RESOLUTION) -> torch.Tensor:
    """Sky.shader {SUN} behind the clouds plane (Sky.shader:707-715): zero where the clouds' alpha is >= 0.5 -> float32 [size, size, 4]"""
    assert clouds.dtype == torch.float32 and clouds.is_contiguous() and clouds.dim() == 3 and clouds.shape[2] == 4, (clouds.dtype, tuple(clouds.shape))
    out = torch.empty((size, size, 4), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_sky_sun_clouds", C.byref(frame), C.byref(params), _ptr(clouds), clouds.shape[1], clouds.shape[0], _ptr(out), size, size)
    return out


def sky_blit_clouds(ctx: "HipContext", clouds: torch.Tensor, target: torch.Tensor, width: int, height: int, band: Band | None = None) -> torch.Tensor:
    """"Blit Clouds" (SkyNode.cpp:722-731): the clouds plane alpha-blended over the rows of `band` of the target, in place; returns `target`"""
    band = band or host.band_whole_frame(width, height)
    assert clouds.dtype == torch.float32 and clouds.is_contiguous() and clouds.dim() == 3 and clouds.shape[2] == 4, (clouds.dtype, tuple(clouds.shape))
    assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (band.fbRowCount, width, 4), tuple(target.shape)
    ctx.call("sailor_hip_sky_blit_clouds", _ptr(clouds), clouds.shape[1], clouds.shape[0], _ptr(target), width, height, C.byref(band))
    return target


def sky_sun_shafts(ctx: "HipContext", frame: UboFrameData, params, clouds: torch.Tensor, target: torch.Tensor, width: int, height: int,
                   band: Band | None = None) -> torch.Tensor:
    """"Sun Shafts" (SkyNode.cpp:733-739): SunShafts.shader blended under the Multiply state over the rows of `band` of the target, in place; returns `target`"""
    band = band or host.band_whole_frame(width, height)
    assert clouds.dtype == torch.float32 and clouds.is_contiguous() and clouds.dim() == 3 and clouds.shape[2] == 4, (clouds.dtype, tuple(clouds.shape))
    assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (band.fbRowCount, width, 4), tuple(target.shape)
    ctx.call("sailor_hip_sky_sun_shafts", C.byref(frame), C.byref(params), _ptr(clouds), clouds.shape[1], clouds.shape[0], _ptr(target), width, height, C.byref(band))
    return target


class SkyStars:
    """The star draw of the Sky node (SkyNode.cpp:694-720).  Holds the mesh of host.sky_star_mesh on the device and the workspace the draw needs; draw()
    binds that workspace to the context and records the two launches."""

    def __init__(self, ctx: "HipContext", positions, colors):
        positions, colors = np.ascontiguousarray(positions, np.float32).reshape(-1, 3), np.ascontiguousarray(colors, np.float32).reshape(-1, 4)
        assert positions.shape[0] == colors.shape[0], (positions.shape, colors.shape)
        self.ctx, self.count = ctx, positions.shape[0]
        # (an empty tensor has no storage: a count of 0 keeps one element so that the pointers are real)
        self.positions = torch.from_numpy(np.concatenate([positions.reshape(-1), np.zeros(3, np.float32)])).to(ctx.device)
        self.colors = torch.from_numpy(np.concatenate([colors.reshape(-1), np.zeros(4, np.float32)])).to(ctx.device)
        self.workspace = torch.empty(max(16, int(ctx._lib.sailor_hip_sky_stars_workspace_bytes(self.count))), dtype=torch.uint8, device=ctx.device)

    def draw(self, frame: UboFrameData, model, clouds: torch.Tensor | None, target: torch.Tensor, width: int, height: int, band: Band | None = None) -> torch.Tensor:
        """adds the stars to the rows of `band` of the target, in place; `clouds` = None is the cleared clouds target; returns `target`"""
        ctx = self.ctx
        band = band or host.band_whole_frame(width, height)
        assert target.dtype == torch.float32 and target.is_contiguous() and tuple(target.shape) == (band.fbRowCount, width, 4), tuple(target.shape)
        if clouds is not None:
            assert clouds.dtype == torch.float32 and clouds.is_contiguous() and clouds.dim() == 3 and clouds.shape[2] == 4, (clouds.dtype, tuple(clouds.shape))
        cw, ch = (0, 0) if clouds is None else (clouds.shape[1], clouds.shape[0])
        model = np.ascontiguousarray(model, dtype=np.float32).reshape(16)
        ctx.call("sailor_hip_sky_stars_bind_workspace", _ptr(self.workspace), self.workspace.numel())
        ctx.call("sailor_hip_sky_stars", C.byref(frame), model.ctypes.data_as(C.POINTER(C.c_float)), _ptr(self.positions), _ptr(self.colors), self.count, _ptr(clouds),
                 cw, ch, _ptr(target), width, height, C.byref(band))
        return target


def sky_env_face(ctx: "HipContext", camera_position, params, chain: torch.Tensor, size: int, face: int) -> torch.Tensor:
    """one face of g_skyCubemap's level 0 (SkyNode.cpp:764-797), written into the flat RGBA32F chain"""
    cam = np.ascontiguousarray(camera_position, dtype=np.float32).reshape(-1)[:3].copy()
    ctx.call("sailor_hip_sky_env_face", cam.ctypes.data_as(C.POINTER(C.c_float)), C.byref(params), _ptr(chain), size, face)
    return chain


def sky_env_cubemap(ctx: "HipContext", camera_position, params, size: int = _lib.SKY_ENV_CUBEMAP_SIZE, levels: int = _lib.SKY_ENV_CUBEMAP_LEVELS) -> torch.Tensor:
    """g_skyCubemap in one call (six faces + GenerateMipMaps, SkyNode.cpp:749-818) -> the flat RGBA32F chain"""
    cam = np.ascontiguousarray(camera_position, dtype=np.float32).reshape(-1)[:3].copy()
    chain = torch.zeros(cube_chain_floats(size, levels), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_sky_env_cubemap", cam.ctypes.data_as(C.POINTER(C.c_float)), C.byref(params), _ptr(chain), size, levels)
    return chain


class Bloom:
    """The Bloom node over a `Main` mip chain (BloomNode.cpp:21-144).  Owns nothing but the parameters: the caller hands in the flat level-major RGBA32F
    chain (host.mip_chain_texels(width, height, levels) * 4 floats, level 0 = the lit frame) and, optionally, the decoded lens-dirt texels [H, W, 4]."""

    def __init__(self, ctx: "HipContext", width: int, height: int, levels: int = _lib.BLOOM_SHIPPED_LEVELS, params=None, dirt: torch.Tensor | None = None):
        self.ctx, self.width, self.height, self.levels = ctx, width, height, levels
        self.params = params if params is not None else host.bloom_params()
        if dirt is not None:
            assert dirt.dtype == torch.float32 and dirt.is_contiguous() and dirt.dim() == 3 and dirt.shape[2] == 4, (dirt.dtype, tuple(dirt.shape))
        self.dirt = dirt
        self.extents = host.mip_chain_extents(width, height, levels)
        self.offsets = [host.mip_chain_texels(width, height, l) * 4 for l in range(levels + 1)]  # in floats

    def chain_floats(self) -> int:
        return self.offsets[-1]

    def level(self, chain: torch.Tensor, l: int) -> torch.Tensor:
        """level l of the chain as a [h, w, 4] view"""
        w, h = self.extents[l]
        return chain[self.offsets[l]:self.offsets[l + 1]].view(h, w, 4)

    def _check(self, chain: torch.Tensor):
        assert chain.dtype == torch.float32 and chain.is_contiguous() and chain.numel() == self.chain_floats(), (chain.dtype, chain.numel(), self.chain_floats())

    def _dirt_args(self):
        return (_ptr(self.dirt), self.dirt.shape[1], self.dirt.shape[0]) if self.dirt is not None else (None, 0, 0)

    def downscale(self, chain: torch.Tensor, i: int) -> None:
        """one Dispatch of the downscale loop: level i -> i + 1 (threshold on for i == 0)"""
        self._check(chain)
        (sw, sh), (dw, dh) = self.extents[i], self.extents[i + 1]
        t = host.bloom_push_constants(self.params.threshold, self.params.knee)
        self.ctx.call("sailor_hip_bloom_downscale", _ptr(self.level(chain, i)), sw, sh, _ptr(self.level(chain, i + 1)), dw, dh, t.ctypes.data_as(C.POINTER(C.c_float)),
                      1 if i == 0 else 0)

    def upscale(self, chain: torch.Tensor, i: int) -> None:
        """one Dispatch of the upscale loop: level i added to level i - 1"""
        self._check(chain)
        (sw, sh), (dw, dh) = self.extents[i], self.extents[i - 1]
        self.ctx.call("sailor_hip_bloom_upscale", _ptr(self.level(chain, i)), sw, sh, _ptr(self.level(chain, i - 1)), dw, dh, i, self.params.bloomIntensity,
                      self.params.dirtIntensity, *self._dirt_args())

    def run(self, chain: torch.Tensor) -> torch.Tensor:
        """the node's whole Process, in place; records only"""
        self._check(chain)
        self.ctx.call("sailor_hip_bloom", _ptr(chain), self.width, self.height, self.levels, C.byref(self.params), *self._dirt_args())
        return chain


def ecs_range_for_rank(n: int, rank: int, world: int):
    """(begin, end, words per rank) of rank's slice of an equal split of n entities in whole visibility words (sailor_hip_ecs_range_for_rank; pure host
    arithmetic, no device)"""
    b, e, per = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _lib.call("sailor_hip_ecs_range_for_rank", n, rank, world, C.byref(b), C.byref(e), C.byref(per))
    return int(b.value), int(e.value), int(per.value)


def _scene_trace(trace: str, octree_root_size: int | None, inserted: torch.Tensor | None) -> _lib.SceneTrace:
    mode = _lib.trace_mode(trace)
    if mode == _lib.TRACE_FLAT_FLOAT_BOXES and (octree_root_size is not None or inserted is not None):
        raise ValueError("octree_root_size and inserted words belong to trace='octree'")
    return _lib.SceneTrace(mode, 0 if octree_root_size is None else octree_root_size, _ptr(inserted))


class EcsSweep:
    """K4 on one GPU over level-sorted entities.  rank / world: this GPU sweeps its slice of an equal split only (sailor_hip_ecs_range_for_rank; one rank of
    one has every entity); the visibility buffer then has room for every rank's words and exchange_visibility() completes it.
    trace: "flat" tests the float world boxes (the default: sailor_hip_ecs_sweep_traced without a trace, what sailor_hip_ecs_sweep runs); "octree" gives
    RHISceneView::TraceScene's set as the reference computes it over integer-truncated boxes and fills `.inserted` (one bit per entity: in the octree at
    all) as well; octree_root_size: the root's size (None = SceneView.h's 264 576).  The matrices and boxes are the same in both modes.  With world > 1
    each rank's `.inserted` holds its own slice's words only: exchange_visibility() gathers the visibility words, not the inserted ones."""

    def __init__(self, ctx: HipContext, entities, rank: int = 0, world: int = 1, trace: str = "flat", octree_root_size: int | None = None):
        _scene_trace(trace, octree_root_size, None)  # an unknown mode raises before anything is allocated
        self.ctx = ctx
        dev = ctx.device
        self.n = len(entities.parent)
        self.rank, self.world_size = rank, world
        self.begin, self.end, self.words_per_rank = ecs_range_for_rank(self.n, rank, world)
        self.trs = torch.from_numpy(entities.transforms).to(dev)
        self.parent = torch.from_numpy(entities.parent.view(np.int32)).to(dev)
        self.local_aabb = torch.from_numpy(entities.local_aabb).to(dev)
        self.level_offsets = np.ascontiguousarray(entities.level_offsets, np.uint32)
        self.world = torch.empty((self.n, 16), dtype=torch.float32, device=dev)
        self.world_aabb = torch.empty((self.n, 6), dtype=torch.float32, device=dev)
        self.visibility = torch.zeros(max((self.n + 63) // 64, world * self.words_per_rank), dtype=torch.int64, device=dev)
        self.trace = trace
        self.inserted = torch.zeros_like(self.visibility) if trace == "octree" else None
        self._trace = _scene_trace(trace, octree_root_size, self.inserted)

    def run(self, planes: np.ndarray):
        planes = np.ascontiguousarray(planes, np.float32).reshape(24)
        self.ctx.call("sailor_hip_ecs_sweep_traced", self.n, _ptr(self.trs), _ptr(self.parent), self.level_offsets.ctypes.data_as(C.POINTER(C.c_uint32)),
                      len(self.level_offsets) - 1, _ptr(self.local_aabb), planes.ctypes.data_as(C.POINTER(C.c_float)), _ptr(self.world), _ptr(self.world_aabb),
                      _ptr(self.visibility), self.begin, self.end, C.byref(self._trace) if self.trace != "flat" else None)
        return self.world, self.world_aabb, self.visibility

    def exchange_visibility(self, comm=None, group=None):
        """every rank's visibility words -> the whole bitmask on every rank: sailor_hip_exchange_visibility on an ncclComm_t (dist.RcclComm), or the same
        all-gather over torch.distributed when there is none (gloo tests, ranks sharing a GPU)"""
        if self.world_size == 1:
            return self.visibility
        if comm is not None:
            self.ctx.call("sailor_hip_exchange_visibility", comm.handle, self.rank, self.world_size, self.n, _ptr(self.visibility), self.visibility.numel())
        else:
            from . import dist as sdist
            sdist.allgather_visibility(self.visibility, self.rank, self.world_size, self.words_per_rank, group)
        return self.visibility


def raster_depth(ctx: "HipContext", light_matrix, positions: torch.Tensor, indices: torch.Tensor, models: torch.Tensor, width: int, height: int,
                 instance_ids: torch.Tensor | None = None, depth: torch.Tensor | None = None, coarse: torch.Tensor | None = None,
                 cull_back: bool = False) -> torch.Tensor:
    """sailor_hip_raster_depth: the caster draws of one shadow pass -> float32 [height, width] depth (reversed Z, 0 = nothing drawn).
    `depth` given = draw on top of it (a dependent pass); otherwise a cleared buffer is used.  `coarse`: int32 [sailor_hip_raster_coarse_words(w, h)] scratch that
    belongs to the depth buffer (hierarchical depth; same result, much less fill)."""
    lm = np.ascontiguousarray(light_matrix, np.float32).reshape(16)
    out = depth if depth is not None else torch.empty((height, width), dtype=torch.float32, device=ctx.device)
    n = models.shape[0] if instance_ids is None else instance_ids.numel()
    ctx.call("sailor_hip_raster_depth", lm.ctypes.data_as(C.POINTER(C.c_float)), _ptr(positions), _ptr(indices), indices.numel() // 3, _ptr(models), _ptr(instance_ids),
             n, width, height, _ptr(out), (0 if depth is not None else _lib.RASTER_CLEAR) | (_lib.RASTER_CULL_BACK if cull_back else 0), _ptr(coarse))
    return out


def raster_depth_camera(ctx: "HipContext", frame, positions: torch.Tensor, indices: torch.Tensor, models: torch.Tensor, width: int, height: int,
                        instance_ids: torch.Tensor | None = None, coarse: torch.Tensor | None = None, cull_back: bool = False) -> torch.Tensor:
    """sailor_hip_raster_depth_camera: the depth prepass -> raw reversed-Z depth float32 [height, width] (0 = nothing drawn)"""
    out = torch.empty((height, width), dtype=torch.float32, device=ctx.device)
    n = models.shape[0] if instance_ids is None else instance_ids.numel()
    ctx.call("sailor_hip_raster_depth_camera", C.byref(frame), _ptr(positions), _ptr(indices), indices.numel() // 3, _ptr(models), _ptr(instance_ids), n, width, height,
             _ptr(out), _lib.RASTER_CLEAR | (_lib.RASTER_CULL_BACK if cull_back else 0), _ptr(coarse))
    return out


def shadow_resolve(ctx: "HipContext", depth: torch.Tensor, fmt: int) -> torch.Tensor:
    """ShadowCaster.shader's fragment stage on the winning depths: RGBA32F EVSM moments, R16F or R32F depth"""
    h, w = depth.shape
    if fmt == _lib.SHADOWMAP_RGBA32F:
        out = torch.empty((h, w, 4), dtype=torch.float32, device=ctx.device)
    elif fmt == _lib.SHADOWMAP_R16F:
        out = torch.empty((h, w), dtype=torch.float16, device=ctx.device)
    else:
        out = torch.empty((h, w), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_shadow_resolve", _ptr(depth), w, h, fmt, _ptr(out))
    return out


def csm_caster_masks(ctx: "HipContext", world_aabb: torch.Tensor, cascade_planes: np.ndarray, trace: str = "flat", octree_root_size: int | None = None,
                     inserted: torch.Tensor | None = None) -> torch.Tensor:
    """sailor_hip_csm_caster_masks: world AABBs [n, 6] (the ECS sweep's output) x cascade frusta [k, 6, 4] -> int64 [k, ceil(n / 64)] bitmasks.
    trace="octree": LightingECS.cpp:296's TraceScene(frustums[k], true) through the octree of integer boxes (sailor_hip_csm_caster_masks_traced);
    `inserted` (int64 [ceil(n / 64)], octree only) then receives the in-the-octree bits."""
    tr = _scene_trace(trace, octree_root_size, inserted)
    pl = np.ascontiguousarray(cascade_planes, np.float32).reshape(-1, 24)
    n = world_aabb.shape[0]
    if inserted is not None and not (inserted.dtype == torch.int64 and inserted.is_contiguous() and inserted.numel() >= (n + 63) // 64):
        raise ValueError(f"inserted must be a contiguous int64 tensor of at least {(n + 63) // 64} words")
    out = torch.empty((len(pl), (n + 63) // 64), dtype=torch.int64, device=ctx.device)  # every word is written
    if trace == "flat":
        ctx.call("sailor_hip_csm_caster_masks", n, _ptr(world_aabb), pl.ctypes.data_as(C.POINTER(C.c_float)), len(pl), _ptr(out))
    else:
        ctx.call("sailor_hip_csm_caster_masks_traced", n, _ptr(world_aabb), pl.ctypes.data_as(C.POINTER(C.c_float)), len(pl), _ptr(out), C.byref(tr))
    return out


def shadow_extract_positions(ctx: "HipContext", vertices: torch.Tensor) -> torch.Tensor:
    """sailor_hip_shadow_extract_positions: the 72-byte vertices of a scene (any contiguous tensor of 72 n bytes) -> float32 [n, 3] positions, what
    raster_depth draws from"""
    n = vertices.numel() * vertices.element_size() // 72
    if not vertices.is_contiguous() or vertices.numel() * vertices.element_size() != 72 * n:
        raise ValueError("vertices must be a contiguous tensor of whole 72-byte records")
    out = torch.empty((n, 3), dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_shadow_extract_positions", _ptr(vertices), n, _ptr(out))
    return out


def shadow_gather_instances_batched(ctx: "HipContext", instances: torch.Tensor, jobs, workspace: torch.Tensor | None = None) -> torch.Tensor | None:
    """sailor_hip_shadow_gather_instances_batched: `instances` = the scene's 96-byte PerInstanceData records (any contiguous tensor of 96 n bytes);
    jobs = [(mask int64 words, begin, end, out float32 [capacity, 16], count int32 [1]), ...] -- passes x batches in one call.  Per job, out[j] = the
    model matrix of the j-th set bit of [begin, end), ascending; count = the set bits of the range, also where `out` is shorter.  Records only.
    Returns the workspace it used (pass it back in to allocate nothing)."""
    n = instances.numel() * instances.element_size() // 96
    if not instances.is_contiguous() or instances.numel() * instances.element_size() != 96 * n:
        raise ValueError("instances must be a contiguous tensor of whole 96-byte records")
    arr = (_lib.ShadowGatherJob * max(len(jobs), 1))()
    for k, (mask, begin, end, out, count, *cap) in enumerate(jobs):   # (a sixth entry: a capacity below the rows of `out`)
        if not (mask.dtype == torch.int64 and mask.is_contiguous() and mask.numel() >= (end + 63) // 64):
            raise ValueError(f"job {k}: mask must be a contiguous int64 tensor of at least {(end + 63) // 64} words")
        if not (out.dtype == torch.float32 and out.is_contiguous() and out.numel() % 16 == 0 and count.dtype == torch.int32 and count.numel() >= 1):
            raise ValueError(f"job {k}: out must be contiguous float32 [capacity, 16] and count int32 [1]")
        if cap and not 0 <= cap[0] <= out.numel() // 16:
            raise ValueError(f"job {k}: capacity {cap[0]} exceeds the {out.numel() // 16} matrices of out")
        arr[k] = _lib.ShadowGatherJob(mask.data_ptr(), begin, end, out.data_ptr(), cap[0] if cap else out.numel() // 16, 0, count.data_ptr())
    need = int(ctx._lib.sailor_hip_shadow_gather_workspace_bytes(arr, len(jobs)))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=ctx.device)
    ctx.call("sailor_hip_shadow_gather_instances_batched", _ptr(instances), n, arr, len(jobs), _ptr(workspace), workspace.numel() * workspace.element_size())
    return workspace


def shadow_gather_instances(ctx: "HipContext", instances: torch.Tensor, mask: torch.Tensor, begin: int, end: int, capacity: int | None = None,
                            workspace: torch.Tensor | None = None):
    """One job of the above into fresh tensors: (models float32 [capacity, 16], count int32 [1]); capacity defaults to end - begin"""
    cap = max(end - begin, 0) if capacity is None else capacity
    out = torch.empty((cap, 16), dtype=torch.float32, device=ctx.device)
    count = torch.empty(1, dtype=torch.int32, device=ctx.device)
    job = _lib.ShadowGatherJob(mask.data_ptr(), begin, end, out.data_ptr(), cap, 0, count.data_ptr())
    need = int(ctx._lib.sailor_hip_shadow_gather_workspace_bytes(C.byref(job), 1))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=ctx.device)
    ctx.call("sailor_hip_shadow_gather_instances", _ptr(instances), instances.numel() * instances.element_size() // 96, _ptr(mask), begin, end, _ptr(out), cap, _ptr(count),
             _ptr(workspace), workspace.numel() * workspace.element_size())
    return out, count


def hiz_build(ctx: "HipContext", depth: torch.Tensor, width: int, height: int, levels: int) -> torch.Tensor:
    """DepthHighZNode's loop on the GPU: raw depth [H, W] float32 -> flat level-major min pyramid"""
    total = sum(max(width >> l, 1) * max(height >> l, 1) for l in range(levels))
    out = torch.empty(total, dtype=torch.float32, device=ctx.device)
    ctx.call("sailor_hip_hiz_build", _ptr(depth), depth.shape[1], depth.shape[0], _ptr(out), width, height, levels)
    return out


class MeshCull:
    """ComputeMeshCulling.shader main() (frustum flags + indirect-draw compaction) over resident instance / indirect buffers."""

    def __init__(self, ctx: HipContext, instances: np.ndarray, batches: np.ndarray):
        assert instances.dtype.itemsize == 96
        self.ctx = ctx
        self.n = len(instances)
        self.num_batches = len(batches)
        self.instances = torch.from_numpy(instances.view(np.uint8).reshape(-1).copy()).to(ctx.device)
        self.batches = torch.from_numpy(np.ascontiguousarray(batches, np.uint32).view(np.int32).copy()).to(ctx.device)
        self._dtype = instances.dtype
        self._ws_bytes = int(ctx._lib.sailor_hip_mesh_cull_workspace_bytes(self.n, self.num_batches))
        self.workspace = torch.empty(max(self._ws_bytes, 256), dtype=torch.uint8, device=ctx.device)

    def run(self, frame, num_instances=None, first_instance=0, hiz=None):
        """hiz = (pyramid tensor, width, height, levels) switches the shader's OCCLUSION_CULLING define on"""
        n = self.n - first_instance if num_instances is None else num_instances
        desc = None
        if hiz is not None:
            desc = _lib.HiZDesc(hiz[0].data_ptr(), hiz[1], hiz[2], hiz[3])
        self.ctx.call("sailor_hip_mesh_cull_compact_ex", C.byref(frame), _ptr(self.instances), n, first_instance, _ptr(self.batches), self.num_batches,
                      _ptr(self.workspace), self._ws_bytes, _ref(desc))
        return self.instances, self.batches

    def download(self):
        self.ctx.synchronize()
        # no ndarray.copy() of the record view: it would not carry the records' padding bytes
        return (self.instances.cpu().numpy().view(self._dtype),
                self.batches.cpu().numpy().view(np.uint32).reshape(-1, 5).copy())


class EyeAdaptation:
    """EyeAdaptationNode (FrameGraph/EyeAdaptationNode.cpp:22-221): log-luminance histogram, smoothed average luminance, tone map.
    Owns the node's state -- the `histogram` SSBO and the 1 x 1 average-luminance target -- as one device tensor."""

    def __init__(self, ctx: HipContext, width: int, height: int, defines: str = "UNCHARTED2 LUMINANCE", white_point=(1.4, 1.5, 1.4, 0.0),
                 exposure: float = 1.0, initial_luminance: float = 0.5):
        self.ctx, self.width, self.height = ctx, width, height
        self.flags = _lib.tonemap_flags(defines)
        self.white_point = (C.c_float * 4)(*[float(v) for v in white_point])
        self.exposure = float(exposure)
        words = int(ctx._lib.sailor_hip_eye_adaptation_state_size()) // 4
        self.state = torch.empty(words, dtype=torch.int32, device=ctx.device)
        self.whole = host.band_whole_frame(width, height)
        self.reset(initial_luminance)

    def reset(self, luminance: float = 0.5):
        self.ctx.call("sailor_hip_eye_adaptation_reset", _ptr(self.state), luminance)

    def constants(self, delta_time: float):
        return host.eye_adaptation_constants(self.width, self.height, delta_time)

    def views(self):
        """(counts, luminance): views of the 256 counts and the adapted-luminance word inside the state tensor"""
        counts, lum = C.c_void_p(), C.c_void_p()
        _lib.call("sailor_hip_eye_adaptation_state_views", _ptr(self.state), C.byref(counts), C.byref(lum))
        c0, l0 = (counts.value - self.state.data_ptr()) // 4, (lum.value - self.state.data_ptr()) // 4
        return self.state[c0:c0 + 256], self.state[l0:l0 + 1].view(torch.float32)

    def _check_rows(self, t: torch.Tensor, band: Band):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (band.fbRowCount, self.width, 4), (tuple(t.shape), band)

    def histogram(self, color: torch.Tensor, constants, band: Band | None = None):
        """adds the counts of the band's rows (`color`: rows x width x 4 float32) to the state's"""
        band = band or self.whole
        self._check_rows(color, band)
        self.ctx.call("sailor_hip_luminance_histogram", _ptr(color), self.width, self.height, C.byref(band), C.byref(constants), _ptr(self.state))

    def average(self, constants):
        self.ctx.call("sailor_hip_average_luminance", C.byref(constants), _ptr(self.state))

    def tonemap(self, color: torch.Tensor, out: torch.Tensor | None = None, band: Band | None = None) -> torch.Tensor:
        band = band or self.whole
        self._check_rows(color, band)
        if out is None:
            out = torch.empty_like(color)
        self._check_rows(out, band)
        self.ctx.call("sailor_hip_tonemap", _ptr(color), _ptr(out), self.width, self.height, C.byref(band), self.flags, self.white_point, self.exposure, _ptr(self.state))
        return out

    def run(self, color: torch.Tensor, delta_time: float, out: torch.Tensor | None = None) -> torch.Tensor:
        """the node's whole sequence on a whole frame"""
        self._check_rows(color, self.whole)
        if out is None:
            out = torch.empty_like(color)
        self._check_rows(out, self.whole)
        constants = self.constants(delta_time)
        self.ctx.call("sailor_hip_eye_adaptation", _ptr(color), _ptr(out), self.width, self.height, C.byref(constants), self.flags, self.white_point, self.exposure,
                      _ptr(self.state))
        return out


class Hbao:
    """The HBAO block of the frame graph (DefaultRenderer.renderer:202-264): Blit DepthBuffer -> HalfDepth, HBAO.shader -> AO, HBAO_Blur.shader VERTICAL ->
    TemporaryR8 and HORIZONTAL -> g_AO.  Owns the three intermediates and g_AO; `run` returns g_AO, the plane SailorIblDesc.ao takes when it is
    frame-sized (the default here; `extents=host.hbao_shipped_extents(w, h)` gives the shipped file's square targets).
    `noise`: the noiseSampler texture as decoded linear float4 texels, (nh, nw, 4) float32 on the device."""

    def __init__(self, ctx: HipContext, width: int, height: int, noise: torch.Tensor, params=None, blur_params=None, extents=None):
        self.ctx, self.width, self.height = ctx, width, height
        assert noise.dtype == torch.float32 and noise.is_contiguous() and noise.dim() == 3 and noise.shape[2] == 4, tuple(noise.shape)
        self.noise = noise
        self.params = params or host.hbao_params()
        self.blur_params = blur_params or host.hbao_blur_params()
        self.extents = extents or ((width // 2, width // 2), (width // 2, width // 2), (width, height), (width, height))
        plane = lambda e: torch.empty((e[1], e[0]), dtype=torch.float32, device=ctx.device)
        self.half_depth, self.ao, self.temp, self.g_ao = (plane(e) for e in self.extents)

    def _check_plane(self, t: torch.Tensor):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2, (t.dtype, tuple(t.shape))

    def blit(self, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        self._check_plane(src), self._check_plane(dst)
        self.ctx.call("sailor_hip_blit_nearest", _ptr(src), src.shape[1], src.shape[0], _ptr(dst), dst.shape[1], dst.shape[0])
        return dst

    def hbao(self, frame, depth: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        self._check_plane(depth), self._check_plane(out)
        self.ctx.call("sailor_hip_hbao", C.byref(frame), _ptr(depth), depth.shape[1], depth.shape[0], _ptr(self.noise), self.noise.shape[1], self.noise.shape[0],
                      C.byref(self.params), _ptr(out), out.shape[1], out.shape[0])
        return out

    def blur_pass(self, ao: torch.Tensor, depth: torch.Tensor, out: torch.Tensor, vertical: bool) -> torch.Tensor:
        self._check_plane(ao), self._check_plane(depth), self._check_plane(out)
        self.ctx.call("sailor_hip_hbao_blur_pass", _ptr(ao), ao.shape[1], ao.shape[0], _ptr(depth), depth.shape[1], depth.shape[0], C.byref(self.blur_params), _ptr(out),
                      out.shape[1], out.shape[0], 1 if vertical else 0)
        return out

    def run(self, frame, raw_depth: torch.Tensor) -> torch.Tensor:
        """the four launches on the raw (reversed-Z) depth attachment, height x width float32; returns g_AO"""
        self._check_plane(raw_depth)
        h, a, t, o = self.half_depth, self.ao, self.temp, self.g_ao
        self.ctx.call("sailor_hip_hbao_chain", C.byref(frame), _ptr(raw_depth), raw_depth.shape[1], raw_depth.shape[0], _ptr(h), h.shape[1], h.shape[0], _ptr(self.noise),
                      self.noise.shape[1], self.noise.shape[0], C.byref(self.params), _ptr(a), a.shape[1], a.shape[0], C.byref(self.blur_params), _ptr(t), t.shape[1],
                      t.shape[0], _ptr(o), o.shape[1], o.shape[0])
        return o


class MotionBlur:
    """The MotionBlur PostProcess entry of the frame graph (DefaultRenderer.renderer:322-334; MotionBlur.shader:63-102): `colorSampler` and `depthSampler`
    in, the `color` target out.  Owns its output (height x width RGBA32F); `run` returns it."""

    def __init__(self, ctx: HipContext, width: int, height: int, params=None):
        self.ctx, self.width, self.height = ctx, width, height
        self.params = params or host.motion_blur_params()
        self.out = torch.empty((height, width, 4), dtype=torch.float32, device=ctx.device)

    def run(self, frame, previous_frame, raw_depth: torch.Tensor, color: torch.Tensor) -> torch.Tensor:
        assert raw_depth.dtype == torch.float32 and raw_depth.is_contiguous() and raw_depth.dim() == 2, tuple(raw_depth.shape)
        assert color.dtype == torch.float32 and color.is_contiguous() and color.dim() == 3 and color.shape[2] == 4, tuple(color.shape)
        self.ctx.call("sailor_hip_motion_blur", C.byref(frame), C.byref(previous_frame), _ptr(raw_depth), raw_depth.shape[1], raw_depth.shape[0], _ptr(color),
                      color.shape[1], color.shape[0], C.byref(self.params), _ptr(self.out), self.width, self.height)
        return self.out


class DebugView:
    """The Debug PostProcess entry (DefaultRenderer.renderer:344-353; Debug.shader:115-178) under one of its routed define sets: "" (the scene copy), "AO",
    "LIGHT_TILES", "CASCADES".  Owns its output (height x width RGBA32F); `run` returns it.  Arguments a mode does not read may be None."""

    def __init__(self, ctx: HipContext, width: int, height: int, define: str = ""):
        if define not in _lib.DEBUG_VIEW_MODES:
            raise ValueError(f"no entry point for Debug.shader under {define!r}: expected one of {sorted(_lib.DEBUG_VIEW_MODES)}")
        self.ctx, self.width, self.height, self.mode = ctx, width, height, _lib.DEBUG_VIEW_MODES[define]
        self.out = torch.empty((height, width, 4), dtype=torch.float32, device=ctx.device)

    def run(self, frame, scene: torch.Tensor | None = None, linear_depth: torch.Tensor | None = None, lights_grid: torch.Tensor | None = None,
            culled_lights: torch.Tensor | None = None, ao: torch.Tensor | None = None) -> torch.Tensor:
        for t in (scene, linear_depth, lights_grid, culled_lights, ao):
            assert t is None or t.is_contiguous()
        w = lambda t: 0 if t is None else t.shape[1]
        h = lambda t: 0 if t is None else t.shape[0]
        self.ctx.call("sailor_hip_debug_view", C.byref(frame), self.mode, _ptr(scene), w(scene), h(scene), _ptr(linear_depth), w(linear_depth), h(linear_depth),
                      _ptr(lights_grid), _ptr(culled_lights), _ptr(ao), w(ao), h(ao), _ptr(self.out), self.width, self.height)
        return self.out


def _check_rgba(t: torch.Tensor):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 4, (t.dtype, tuple(t.shape))


class Blur:
    """A Blur.shader PostProcess entry outside the shadow pass (DefaultRenderer.renderer:157-181; Blur.shader:66-98): the Gauss blur under "", "HORIZONTAL",
    "VERTICAL" or both, the radial one under any set with "RADIAL".  `colorSampler` (any extent) in, the `color` target out.  Owns its output (height x width
    RGBA32F; the Gauss blur writes alpha 0); `run` returns it."""

    def __init__(self, ctx: HipContext, width: int, height: int, defines: str = "", params=None):
        self.ctx, self.width, self.height, self.flags = ctx, width, height, _lib.blur_flags(defines)
        self.params = params or host.blur_params(**(_lib.BLUR_RADIAL_SHIPPED if self.flags & _lib.BLUR_RADIAL else _lib.BLUR_GAUSS_SHIPPED))
        self.out = torch.empty((height, width, 4), dtype=torch.float32, device=ctx.device)

    def run(self, color: torch.Tensor) -> torch.Tensor:
        _check_rgba(color)
        self.ctx.call("sailor_hip_blur", _ptr(color), color.shape[1], color.shape[0], C.byref(self.params), self.flags, _ptr(self.out), self.width, self.height)
        return self.out


class ChromaticAberration:
    """The ChromaticAberation.shader PostProcess entry (DefaultRenderer.renderer:355-366; ChromaticAberation.shader:62-73): `colorSampler` (any extent) in, the
    `color` target out.  Owns its output (height x width RGBA32F, alpha 1); `run` returns it."""

    def __init__(self, ctx: HipContext, width: int, height: int, params=None):
        self.ctx, self.width, self.height = ctx, width, height
        self.params = params or host.chromatic_aberration_params()
        self.out = torch.empty((height, width, 4), dtype=torch.float32, device=ctx.device)

    def run(self, color: torch.Tensor) -> torch.Tensor:
        _check_rgba(color)
        self.ctx.call("sailor_hip_chromatic_aberration", _ptr(color), color.shape[1], color.shape[0], C.byref(self.params), _ptr(self.out), self.width, self.height)
        return self.out


def blit_linear(ctx: HipContext, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """The Blit entry of a scaled image with Linear filtration (BlitNode.cpp:88-96): src -> dst, both (h, w, 4) RGBA32F or both (h, w) one-channel fp32"""
    assert src.dtype == dst.dtype == torch.float32 and src.is_contiguous() and dst.is_contiguous(), (src.dtype, dst.dtype)
    assert src.dim() == dst.dim() and (src.dim() == 2 or (src.dim() == 3 and src.shape[2] == dst.shape[2] == 4)), (tuple(src.shape), tuple(dst.shape))
    ctx.call("sailor_hip_blit_linear", _ptr(src), src.shape[1], src.shape[0], _ptr(dst), dst.shape[1], dst.shape[0], 4 if src.dim() == 3 else 1)
    return dst


def upload_textures(ctx: HipContext, images, srgb, mips: bool = False) -> tuple[torch.Tensor, int, list]:
    """Standard.shader:124 textureSamplers[]: a list of uint8 [H, W, 4] arrays (r first) and their sRGB flags -> (device table of SailorTextureDesc, its
    length, the tensors that must stay alive).  mips: allocate the full chain behind every image, upload level 0, record sailor_hip_texture_generate_mips and
    set the descriptor's `levels` (what the `_lod` entry points read); without it the descriptors hold one level, as before."""
    assert len(images) == len(srgb) and len(images) > 0
    keep, table = [], (_lib.TextureDesc * len(images))()
    for k, (img, s) in enumerate(zip(images, srgb)):
        img = np.ascontiguousarray(img, np.uint8)
        assert img.ndim == 3 and img.shape[2] == 4 and img.shape[0] > 0 and img.shape[1] > 0, img.shape
        h, w = img.shape[:2]
        flags, levels = _lib.TEXTURE_SRGB if s else 0, 0
        t = torch.from_numpy(img.view(np.uint32).reshape(h, w).view(np.int32)).to(ctx.device)
        if mips:
            levels = host.texture_mip_levels(w, h)
            chain = torch.zeros(host.mip_chain_texels(w, h, levels), dtype=torch.int32, device=ctx.device)
            chain[: h * w] = t.reshape(-1)
            t = chain
            ctx.call("sailor_hip_texture_generate_mips", _ptr(t), w, h, levels, flags)
        keep.append(t)
        table[k] = _lib.TextureDesc(t.data_ptr(), w, h, flags, levels)
    d = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(ctx.device)
    keep.append(d)
    return d, len(images), keep


class SurfacePass:
    """RenderScene's producer of the surface buffer (sailor_hip_surface_*): begin -> draw per DrawIndexed -> resolve -> the shade -> composite.  Owns the
    workspace (keys and draw descriptors) and the running primBase / drawIndex."""

    def __init__(self, ctx: HipContext, width: int, height: int, band: Band | None = None, max_draws: int = 64):
        self.ctx, self.W, self.H = ctx, width, height
        self.band = band if band is not None else host.band_whole_frame(width, height)
        self.rows = self.band.fbRowCount
        n = ctx._lib.sailor_hip_surface_workspace_bytes(width, height, C.byref(self.band), max_draws)
        if n == 0:
            raise _lib.SailorHipError(-1, "sailor_hip_surface_workspace_bytes")
        self.workspace = torch.empty(n, dtype=torch.uint8, device=ctx.device)
        self.prim_base = self.draw_index = 0

    # -- what every entry of the pass takes, built in one place each -------------------------------------------------------
    def _frame_args(self):
        """(W, H, band, workspace, its bytes): the frame arguments of the pass's entries"""
        return self.W, self.H, C.byref(self.band), _ptr(self.workspace), self.workspace.numel()

    @staticmethod
    def _table_args(instances, materials, textures, num_textures):
        """(instances, materials, their count of 80-byte records, textures, their count): the table arguments of the draws and the resolves"""
        return _ptr(instances), _ptr(materials), 0 if materials is None else materials.numel() * materials.element_size() // 80, _ptr(textures), num_textures

    @staticmethod
    def _draw_desc(d: dict, instances: torch.Tensor, prim_base: int, blend: bool = False):
        """a draw's keyword arguments (draw()'s: vertices, indices, instance_ids, num_drawn, first_instance, cull_back, alpha_cutout, gltf; with `blend`
        also its blend mode) -> (its SailorSurfaceDraw at prim_base, the primitives it advances the pass's primBase by)"""
        ids, first, drawn = d.get("instance_ids"), d.get("first_instance", 0), d.get("num_drawn")
        if drawn is None:
            drawn = ids.numel() if ids is not None else instances.numel() * instances.element_size() // 96 - first
        nt = d["indices"].numel() // 3
        flags = (_lib.SURFACE_CULL_BACK if d.get("cull_back", False) else 0) | (_lib.SURFACE_ALPHA_CUTOUT if d.get("alpha_cutout", False) else 0) | \
                (_lib.SURFACE_GLTF if d.get("gltf", False) else 0)
        if blend:
            mode = d.get("blend", "none")
            flags |= (_lib.SURFACE_BLEND_MODES[mode] if isinstance(mode, str) else int(mode)) << _lib.SURFACE_BLEND_SHIFT
        return _lib.SurfaceDraw(_ptr(d["vertices"]), _ptr(d["indices"]), _ptr(ids), nt, drawn, prim_base, flags, first, 0), host.surface_draw_prims(nt, drawn)

    def _draw_descs(self, draws, instances: torch.Tensor, prim_base: int, blend: bool = False):
        """the descriptors of a pass recorded from dicts, with the running primBase; leaves prim_base / draw_index behind the last of them"""
        descs = []
        for d in draws:
            desc, prims = self._draw_desc(d, instances, prim_base, blend)
            descs.append(desc)
            prim_base += prims
        self.prim_base, self.draw_index = prim_base, len(descs)
        return descs

    @staticmethod
    def _draw_entry(route: str, desc) -> str:
        """the draw entry of a route ("peel", "bucket", "msaa"): Standard.shader's, or Standard_glTF.shader's by the descriptor's flag"""
        return f"sailor_hip_surface_{route}_draw_gltf" if desc.flags & _lib.SURFACE_GLTF else f"sailor_hip_surface_{route}_draw"

    def _shade_layer(self, k: int, frame, scene, any_gltf: bool, ao_in, shade, on_layer, weight: torch.Tensor | None = None):
        """The layer step: the layer in the workspace resolved (resolve_gltf if the pass holds a glTF draw) -> on_layer -> shade -> (surface, radiance,
        emissive | None).  scene: (instances, materials, textures, num_textures).  on_layer's third argument is `weight` or, without one, the coverage."""
        want_coverage = on_layer is not None and weight is None
        if any_gltf:
            surface, _, cov, ao, emissive = self.resolve_gltf(frame, *scene, ao_in=ao_in, want_depth=False, want_coverage=want_coverage)
        else:
            surface, _, cov = self.resolve(frame, *scene, want_depth=False, want_coverage=want_coverage)
            ao, emissive = ao_in, None
        if on_layer is not None:
            on_layer(k, surface, cov if weight is None else weight, emissive, ao)
        radiance = shade(surface, ao)
        assert radiance.dtype == torch.float32 and radiance.shape == (self.rows, self.W, 4) and radiance.is_contiguous()
        return surface, radiance, emissive

    def begin(self, depth: torch.Tensor | None = None, prim_base: int = 0):
        """depth: the prepass's raw depth of the WHOLE frame, float32 [H, W], or None"""
        assert depth is None or (depth.dtype == torch.float32 and depth.shape == (self.H, self.W) and depth.is_contiguous())
        self.ctx.call("sailor_hip_surface_begin", _ptr(depth), *self._frame_args())
        self.prim_base, self.draw_index = prim_base, 0

    def draw(self, frame: UboFrameData, vertices: torch.Tensor, indices: torch.Tensor, instances: torch.Tensor, instance_ids: torch.Tensor | None = None,
             num_drawn: int | None = None, first_instance: int = 0, cull_back: bool = False, alpha_cutout: bool = False, materials: torch.Tensor | None = None,
             textures: torch.Tensor | None = None, num_textures: int = 0, gltf: bool = False, lod: bool = False):
        """vertices: 72-byte records; indices: int32, 3 per triangle; instances: the 96-byte PerInstanceData SSBO; instance_ids: int32 or None.
        lod: through sailor_hip_surface_draw_lod -- the alpha behind ALPHA_CUTOUT is fetched at the implicit level of detail; such a pass ends with resolve_lod.
        alpha_cutout: the ALPHA_CUTOUT permutation (Standard.shader:403-408) through sailor_hip_surface_draw_masked, which needs the resolve's material and
        texture tables.  gltf: the draw's material is Standard_glTF.shader's (sailor_hip_surface_draw_gltf); such a pass ends with resolve_gltf / composite_gltf"""
        d, prims = self._draw_desc(dict(vertices=vertices, indices=indices, instance_ids=instance_ids, num_drawn=num_drawn, first_instance=first_instance,
                                        cull_back=cull_back, alpha_cutout=alpha_cutout, gltf=gltf), instances, self.prim_base)
        if lod or gltf or alpha_cutout:
            name = "sailor_hip_surface_draw_lod" if lod else "sailor_hip_surface_draw_gltf" if gltf else "sailor_hip_surface_draw_masked"
            self.ctx.call(name, C.byref(frame), C.byref(d), *self._table_args(instances, materials, textures, num_textures), self.draw_index, *self._frame_args())
        else:
            self.ctx.call("sailor_hip_surface_draw", C.byref(frame), C.byref(d), _ptr(instances), self.draw_index, *self._frame_args())
        self.prim_base += prims
        self.draw_index += 1

    def draw_indirect(self, frame: UboFrameData, vertices: torch.Tensor, indices: torch.Tensor, instances: torch.Tensor, command: torch.Tensor, capacity: int,
                      command_index: int = 0, num_instance_records: int | None = None, cull_back: bool = False, alpha_cutout: bool = False,
                      materials: torch.Tensor | None = None, textures: torch.Tensor | None = None, num_textures: int = 0, gltf: bool = False, lod: bool = False):
        """One command of DrawIndexedIndirect (sailor_hip_surface_draw_indirect; lod: sailor_hip_surface_draw_indirect_lod, as in draw()).  command: the device buffer of 20-byte DrawIndexedIndirectData, e.g.
        MeshCull's `batches`; command_index: which of them.  capacity: the instanceCount the host wrote (the un-culled count); the kernel reads the count
        and firstInstance of the command when it runs, and the running primBase advances by the capacity.  num_instance_records: the records `instances`
        holds for the draw's guard (default: all of the tensor)."""
        if num_instance_records is None:
            num_instance_records = instances.numel() * instances.element_size() // 96
        d, prims = self._draw_desc(dict(vertices=vertices, indices=indices, num_drawn=capacity, cull_back=cull_back, alpha_cutout=alpha_cutout, gltf=gltf), instances,
                                   self.prim_base)
        d_instances, *tables = self._table_args(instances, materials, textures, num_textures)
        self.ctx.call("sailor_hip_surface_draw_indirect_lod" if lod else "sailor_hip_surface_draw_indirect", C.byref(frame), C.byref(d),
                      command.data_ptr() + 20 * command_index, d_instances, num_instance_records, *tables, self.draw_index, *self._frame_args())
        self.prim_base += prims
        self.draw_index += 1

    def store_depth(self, depth: torch.Tensor) -> torch.Tensor:
        """the keys' depth into the band's rows of `depth`, the raw depth attachment of the WHOLE frame, float32 [H, W]: the depth write of a pass that held
        cutout draws"""
        assert depth.dtype == torch.float32 and depth.shape == (self.H, self.W) and depth.is_contiguous()
        self.ctx.call("sailor_hip_surface_store_depth", _ptr(self.workspace), self.workspace.numel(), _ptr(depth), self.W, self.H, C.byref(self.band))
        return depth

    def resolve(self, frame: UboFrameData, instances: torch.Tensor, materials: torch.Tensor, textures: torch.Tensor, num_textures: int, want_depth: bool = True,
                want_coverage: bool = True):
        """-> (surface float32 [3, rows, W, 4], depth float32 [rows, W] | None, coverage uint8 [rows, W] | None)"""
        dev = self.ctx.device
        surface = torch.empty((3, self.rows, self.W, 4), dtype=torch.float32, device=dev)
        depth = torch.empty((self.rows, self.W), dtype=torch.float32, device=dev) if want_depth else None
        cov = torch.empty((self.rows, self.W), dtype=torch.uint8, device=dev) if want_coverage else None
        self.ctx.call("sailor_hip_surface_resolve", C.byref(frame), *self._table_args(instances, materials, textures, num_textures), *self._frame_args(), _ptr(surface),
                      self.rows * self.W, _ptr(depth), _ptr(cov))
        return surface, depth, cov

    def composite(self, radiance: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """target = covered ? radiance : target; both float32 [rows, W, 4]"""
        for t in (radiance, target):
            assert t.dtype == torch.float32 and t.shape == (self.rows, self.W, 4) and t.is_contiguous()
        self.ctx.call("sailor_hip_surface_composite", _ptr(radiance), _ptr(self.workspace), self.workspace.numel(), _ptr(target), self.W, self.H, C.byref(self.band))
        return target

    def resolve_lod(self, frame: UboFrameData, instances: torch.Tensor, materials: torch.Tensor, textures: torch.Tensor, num_textures: int,
                    ao_in: torch.Tensor | None = None, want_depth: bool = True, want_coverage: bool = True, want_ao: bool = True):
        """resolve_gltf() with every fetch at its implicit level of detail (sailor_hip_surface_resolve_lod); a table of one-level descriptors gives
        resolve_gltf()'s bits"""
        return self.resolve_gltf(frame, instances, materials, textures, num_textures, ao_in, want_depth, want_coverage, want_ao, entry="sailor_hip_surface_resolve_lod")

    def resolve_gltf(self, frame: UboFrameData, instances: torch.Tensor, materials: torch.Tensor, textures: torch.Tensor, num_textures: int,
                     ao_in: torch.Tensor | None = None, want_depth: bool = True, want_coverage: bool = True, want_ao: bool = True,
                     entry: str = "sailor_hip_surface_resolve_gltf"):
        """resolve() for a pass that may hold glTF draws.  ao_in: g_AO over the band, float32 [rows, W], or None (1 everywhere).
        -> (surface, depth | None, coverage | None, ao_out float32 [rows, W] | None -- what the shade reads as its IBL desc's ao --, emissive float32 [rows, W, 4])"""
        dev = self.ctx.device
        assert ao_in is None or (ao_in.dtype == torch.float32 and ao_in.shape == (self.rows, self.W) and ao_in.is_contiguous())
        surface = torch.empty((3, self.rows, self.W, 4), dtype=torch.float32, device=dev)
        depth = torch.empty((self.rows, self.W), dtype=torch.float32, device=dev) if want_depth else None
        cov = torch.empty((self.rows, self.W), dtype=torch.uint8, device=dev) if want_coverage else None
        ao_out = torch.empty((self.rows, self.W), dtype=torch.float32, device=dev) if want_ao else None
        emissive = torch.empty((self.rows, self.W, 4), dtype=torch.float32, device=dev)
        self.ctx.call(entry, C.byref(frame), *self._table_args(instances, materials, textures, num_textures), *self._frame_args(), _ptr(surface), self.rows * self.W,
                      _ptr(depth), _ptr(cov), _ptr(ao_in), _ptr(ao_out), _ptr(emissive))
        return surface, depth, cov, ao_out, emissive

    def composite_gltf(self, radiance: torch.Tensor, emissive: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """target = covered ? (emissive.rgb + radiance.rgb, radiance.a) : target; all float32 [rows, W, 4]"""
        for t in (radiance, emissive, target):
            assert t.dtype == torch.float32 and t.shape == (self.rows, self.W, 4) and t.is_contiguous()
        self.ctx.call("sailor_hip_surface_composite_gltf", _ptr(radiance), _ptr(emissive), _ptr(self.workspace), self.workspace.numel(), _ptr(target), self.W, self.H,
                      C.byref(self.band))
        return target

    def transparent(self, frame: UboFrameData, draws, instances: torch.Tensor, materials: torch.Tensor, textures: torch.Tensor, num_textures: int,
                    depth: torch.Tensor, shade, target: torch.Tensor, ao_in: torch.Tensor | None = None, layers: int | None = None, prim_base: int = 0,
                    on_layer=None, mode: str = "peel") -> torch.Tensor:
        """A RenderScene pass with `Tag: Transparent` (the Transparent section of include/sailor_hip.h): depth test against `depth` (the raw depth attachment of
        the WHOLE frame, float32 [H, W], read only), no depth write, every fragment blended onto `target` (float32 [rows, W, 4]) in primitive order.  The pass is
        peeled by primitive order, one layer at a time, and every layer rasterises the draws again.
        draws: dicts of draw()'s keyword arguments (vertices, indices, instance_ids, num_drawn, first_instance, cull_back, alpha_cutout, gltf) plus `blend`:
        "none", "additive" or "alpha" ("multiply" is refused: unsupported).
        shade: a callable (surface float32 [3, rows, W, 4], ao float32 [rows, W] | None) -> radiance float32 [rows, W, 4]: the shade of the opaque pass bound to
        its lights, lists and shadow maps -- e.g. lambda s, ao: fp.shade(frame, s, lights, n).  ao is resolve_gltf's aoOut (None if no draw is glTF's).
        layers=N records N layers and the overflow round, reads nothing back and returns the device counters, int32 [N + 1]: the pixels each layer committed and,
        last, the OVERFLOW -- the pixels that still had a fragment left.  layers=None is for tools and tests and SYNCHRONISES: it reads the committed count
        after each layer and stops at the first empty one (the counters returned end with that 0).
        on_layer(k, surface, coverage, emissive | None, ao | None): called behind every resolve (a test's window into the layers).
        mode: "peel" (the default: the launches above) or "buckets" -- the draws run ONCE into per-pixel fragment buckets (sailor_hip_surface_bucket_*; self.buckets,
        (layers + 1) x 8 bytes a pixel) and every layer is read out of them.  "buckets" requires layers=N, 1 .. 64; the counters, the target's bits and on_layer
        are the peel's."""
        ctx, dev = self.ctx, self.ctx.device
        assert mode in ("peel", "buckets") and (mode == "peel" or layers is not None), "mode='buckets' requires layers=N"
        assert depth.dtype == torch.float32 and depth.shape == (self.H, self.W) and depth.is_contiguous()
        assert target.dtype == torch.float32 and target.shape == (self.rows, self.W, 4) and target.is_contiguous()
        assert layers is None or layers >= 0
        any_gltf = any(d.get("gltf", False) for d in draws)
        scene = (instances, materials, textures, num_textures)
        tables, fa = self._table_args(*scene), self._frame_args()
        self.last = torch.empty((self.rows, self.W), dtype=torch.int32, device=dev)
        descs = self._draw_descs(draws, instances, prim_base, blend=True)

        def peel(k, count):
            ctx.call("sailor_hip_surface_peel_begin", *fa, _ptr(self.last), 1 if k == 0 else 0)
            for index, d in enumerate(descs):
                ctx.call(self._draw_entry("peel", d), C.byref(frame), C.byref(d), *tables, index, *fa, _ptr(depth), _ptr(self.last))
            ctx.call("sailor_hip_surface_peel_commit", *fa, _ptr(self.last), _ptr(count))

        def blend_layer(k):
            surface, radiance, emissive = self._shade_layer(k, frame, scene, any_gltf, ao_in, shade, on_layer)
            ctx.call("sailor_hip_surface_blend", _ptr(radiance), _ptr(surface), _ptr(emissive), _ptr(self.workspace), self.workspace.numel(), _ptr(target), self.W, self.H, C.byref(self.band))

        if mode == "buckets":
            nb = ctx._lib.sailor_hip_surface_bucket_bytes(self.W, C.byref(self.band), layers)
            self.buckets = torch.empty(nb // 8, dtype=torch.int64, device=dev)
            store = (_ptr(self.buckets), nb, layers)
            ctx.call("sailor_hip_surface_bucket_begin", *fa, *store)
            for index, d in enumerate(descs):
                ctx.call(self._draw_entry("bucket", d), C.byref(frame), C.byref(d), *tables, index, *fa, _ptr(depth), *store)
            counts = torch.zeros(layers + 1, dtype=torch.int32, device=dev)
            for k in range(layers + 1):
                ctx.call("sailor_hip_surface_bucket_layer", *fa, *store, k, _ptr(counts[k:]))
                if k < layers:
                    blend_layer(k)
            return counts
        if layers is not None:
            counts = torch.zeros(layers + 1, dtype=torch.int32, device=dev)
            for k in range(layers):
                peel(k, counts[k:])
                blend_layer(k)
            peel(layers, counts[layers:])
            return counts
        counts, k = [], 0
        while True:
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            peel(k, count)
            ctx.synchronize()
            counts.append(count)
            if int(count.item()) == 0:
                return torch.cat(counts)
            blend_layer(k)
            k += 1

    def multisampled(self, frame: UboFrameData, draws, instances: torch.Tensor, materials: torch.Tensor, textures: torch.Tensor, num_textures: int, shade,
                     target: torch.Tensor, samples: int = 8, layers: int | None = None, sample_depth: torch.Tensor | None = None,
                     ao_in: torch.Tensor | None = None, prim_base: int = 0, on_layer=None) -> torch.Tensor:
        """A multisampled RenderScene pass (the Multisampled section of include/sailor_hip.h; sailor_hip_surface_msaa_*): the draws run once into a store of
        `samples` keys a pixel (self.sample_store, samples x 8 bytes a pixel), every layer -- the pixel's primitives in primitive order -- is read out into the
        workspace, resolved and shaded at the pixel centre as ever, and accumulated onto `target` (float32 [rows, W, 4]) with the share of the samples it owns:
        the reference's AVERAGE resolve.  samples: 1, 2, 4 or 8.
        draws: dicts of draw()'s keyword arguments (vertices, indices, instance_ids, num_drawn, first_instance, cull_back, alpha_cutout, gltf).
        shade: the callable of transparent(): (surface float32 [3, rows, W, 4], ao float32 [rows, W] | None) -> radiance float32 [rows, W, 4].
        layers: how many primitives a pixel may show, 1 .. samples (None: samples, which never clips); a pixel with more gives the samples of the others to
        its last layer.  sample_depth: float32 [rows, W, samples], what store_sample_depth() of a multisampled prepass returned, or None.
        Records only and reads nothing back; returns the device counters, int32 [layers + 1]: the pixels each layer holds and, last, the clipped pixels.
        on_layer(k, surface, weight uint8 [rows, W], emissive | None, ao | None): called behind every resolve (a test's window into the layers); the bytes of
        the samples no primitive owns are self.uncovered."""
        ctx, dev = self.ctx, self.ctx.device
        layers = samples if layers is None else layers
        assert target.dtype == torch.float32 and target.shape == (self.rows, self.W, 4) and target.is_contiguous()
        assert sample_depth is None or (sample_depth.dtype == torch.float32 and sample_depth.shape == (self.rows, self.W, samples) and sample_depth.is_contiguous())
        any_gltf = any(d.get("gltf", False) for d in draws)
        scene = (instances, materials, textures, num_textures)
        tables, fa = self._table_args(*scene), self._frame_args()
        nb = ctx._lib.sailor_hip_surface_msaa_bytes(self.W, C.byref(self.band), samples)
        if nb == 0:
            raise _lib.SailorHipError(-1, "sailor_hip_surface_msaa_bytes")
        if getattr(self, "sample_store", None) is None or self.sample_store.numel() * 8 != nb:
            self.sample_store = torch.empty(nb // 8, dtype=torch.int64, device=dev)
        self.samples = samples
        store = (_ptr(self.sample_store), nb, samples)
        ctx.call("sailor_hip_surface_msaa_begin", *fa, *store, _ptr(sample_depth))
        for index, d in enumerate(self._draw_descs(draws, instances, prim_base)):
            ctx.call(self._draw_entry("msaa", d), C.byref(frame), C.byref(d), *tables, index, *fa, *store)
        counts = torch.zeros(layers + 1, dtype=torch.int32, device=dev)
        self.weights = torch.empty((layers, self.rows, self.W), dtype=torch.uint8, device=dev)
        self.uncovered = torch.empty((self.rows, self.W), dtype=torch.uint8, device=dev)
        for k in range(layers):
            weight = self.weights[k]
            ctx.call("sailor_hip_surface_msaa_layer", *fa, *store, layers, k, _ptr(weight), _ptr(self.uncovered) if k == 0 else None, _ptr(counts[k:]),
                     _ptr(counts[layers:]))
            _, radiance, emissive = self._shade_layer(k, frame, scene, any_gltf, ao_in, shade, on_layer, weight)
            ctx.call("sailor_hip_surface_msaa_accumulate", _ptr(radiance), _ptr(emissive), _ptr(weight), _ptr(self.uncovered), samples, k, _ptr(target), self.W, self.H,
                     C.byref(self.band))
        return counts

    def store_sample_depth(self, depth: torch.Tensor | None = None, want_samples: bool = True):
        """the depth of the last multisampled() pass: -> (the sample depths, float32 [rows, W, samples], for the next pass's sample_depth -- None without
        want_samples --, depth).  depth: the raw depth attachment of the WHOLE frame, float32 [H, W], or None; the band's rows of it take the samples' AVERAGE"""
        assert depth is None or (depth.dtype == torch.float32 and depth.shape == (self.H, self.W) and depth.is_contiguous())
        out = torch.empty((self.rows, self.W, self.samples), dtype=torch.float32, device=self.ctx.device) if want_samples else None
        self.ctx.call("sailor_hip_surface_msaa_store_depth", _ptr(self.sample_store), self.sample_store.numel() * 8, self.samples, _ptr(out), _ptr(depth), self.W, self.H,
                      C.byref(self.band))
        return out, depth

    def download_samples(self) -> np.ndarray:
        """the store of the last multisampled() as uint64 [rows, W, samples]: depth bits << 32 | (order + 1)"""
        self.ctx.synchronize()
        return self.sample_store.cpu().numpy().view(np.uint64).reshape(self.rows, self.W, self.samples)

    def download_keys(self) -> np.ndarray:
        """the keys as uint64 [rows, W]: depth bits << 32 | (order + 1)"""
        self.ctx.synchronize()
        at, n = self.ctx._lib.sailor_hip_surface_keys_offset(), self.rows * self.W * 8
        return self.workspace[at: at + n].cpu().numpy().view(np.uint64).reshape(self.rows, self.W)

    def download_buckets(self) -> np.ndarray:
        """the store of the last transparent(mode="buckets") as uint64 [layers + 1, rows, W]: (order + 1) << 32 | depth bits, all ones where a slot is empty"""
        self.ctx.synchronize()
        return self.buckets.cpu().numpy().view(np.uint64).reshape(-1, self.rows, self.W)


def masked_depth_prepass(sp: SurfacePass, frame: UboFrameData, depth: torch.Tensor, draws, instances: torch.Tensor, materials: torch.Tensor, textures: torch.Tensor,
                         num_textures: int) -> torch.Tensor:
    """DepthPrepass with `Tag: Masked` (DepthPrepassNode.cpp:246-255: Standard.shader with ALPHA_CUTOUT against no colour attachment): begin from `depth` (the
    Opaque prepass's raw depth of the whole frame), the masked draws, the keys' depth back into `depth`.  draws: dicts of SurfacePass.draw's keyword arguments
    (vertices, indices, instance_ids, num_drawn, first_instance, cull_back)."""
    sp.begin(depth)
    for d in draws:
        sp.draw(frame, instances=instances, alpha_cutout=True, materials=materials, textures=textures, num_textures=num_textures, **d)
    return sp.store_depth(depth)


class DebugLinesPass:
    """The DebugDraw node's pass (sailor_hip_debug_lines_*): begin from the current DepthBuffer -> the one draw of DebugContext::DrawDebugMesh -> resolve into
    Main and DepthBuffer.  Owns a surface-pass workspace (the keys)."""

    def __init__(self, ctx: HipContext, width: int, height: int, band: Band | None = None):
        self.surface = SurfacePass(ctx, width, height, band, max_draws=1)
        self.ctx, self.W, self.H, self.band, self.rows, self.workspace = ctx, width, height, self.surface.band, self.surface.rows, self.surface.workspace
        self._draw, self._vp = None, None

    def begin(self, depth: torch.Tensor | None):
        """depth: the raw DepthBuffer of the WHOLE frame, float32 [H, W] (or None: keys of 0)"""
        self.surface.begin(depth)
        self._draw = None

    def draw(self, view_projection, vertices: torch.Tensor, indices: torch.Tensor | None = None, num_segments: int | None = None, prim_base: int = 0):
        """view_projection: 16 floats, column-major (the push constant); vertices: 28-byte VertexP3C4 records; indices: int32, 2 per segment, or None"""
        if num_segments is None:
            num_segments = indices.numel() // 2 if indices is not None else vertices.numel() * vertices.element_size() // 56
        self._vp = (C.c_float * 16)(*[float(x) for x in np.asarray(view_projection, np.float32).reshape(16)])
        self._draw = _lib.DebugLinesDraw(_ptr(vertices), _ptr(indices), num_segments, prim_base)
        self.ctx.call("sailor_hip_debug_lines_draw", self._vp, C.byref(self._draw), *self.surface._frame_args())

    def resolve(self, target: torch.Tensor, depth: torch.Tensor):
        """target: float32 [rows, W, 4] (the band's rows of Main); depth: float32 [H, W] (the whole DepthBuffer); both written where a segment owns the pixel"""
        assert self._draw is not None, "resolve() before draw()"
        assert target.dtype == torch.float32 and target.shape == (self.rows, self.W, 4) and target.is_contiguous()
        assert depth.dtype == torch.float32 and depth.shape == (self.H, self.W) and depth.is_contiguous()
        self.ctx.call("sailor_hip_debug_lines_resolve", self._vp, C.byref(self._draw), *self.surface._frame_args(), _ptr(target), _ptr(depth))
        return target, depth

    def download_keys(self) -> np.ndarray:
        return self.surface.download_keys()


class UiPass:
    """The RenderImGui node's pass (sailor_hip_ui_draw): the flattened commands of a frame's draw data blended in primitive order into the band's rows of an
    fp32 RGBA target.  Owns the workspace (grown by reserve(), outside any recorded region) and the font texture's descriptor."""

    def __init__(self, ctx: HipContext, width: int, height: int, band: Band | None = None, max_triangles: int = 0):
        self.ctx, self.W, self.H = ctx, width, height
        self.band = band if band is not None else host.band_whole_frame(width, height)
        self.rows = self.band.fbRowCount
        self.workspace, self.capacity = None, -1
        self._texture, self._keep = _lib.TextureDesc(None, 0, 0, 0, 0), None
        self.reserve(max_triangles)

    def reserve(self, num_triangles: int):
        """a workspace for draws of up to num_triangles triangles (allocates: not inside a capture)"""
        if num_triangles > self.capacity:
            n = C.c_size_t()
            _lib.call("sailor_hip_ui_workspace_bytes", num_triangles, self.W, self.H, C.byref(n))
            self.workspace, self.capacity = torch.empty(n.value, dtype=torch.uint8, device=self.ctx.device), num_triangles

    def set_texture(self, image: np.ndarray | None):
        """the font atlas: uint8 [h, w, 4], r first (R8G8B8A8_UNORM), or None: a descriptor without texels, which samples as 0"""
        if image is None:
            self._texture, self._keep = _lib.TextureDesc(None, 0, 0, 0, 0), None
            return
        img = np.ascontiguousarray(image, np.uint8)
        assert img.ndim == 3 and img.shape[2] == 4 and img.shape[0] > 0 and img.shape[1] > 0, img.shape
        self._keep = torch.from_numpy(img.view(np.uint32).reshape(img.shape[0], img.shape[1]).view(np.int32)).to(self.ctx.device)
        self._texture = _lib.TextureDesc(self._keep.data_ptr(), img.shape[1], img.shape[0], 0, 0)

    def draw(self, target: torch.Tensor, vertices: torch.Tensor, indices: torch.Tensor, commands: np.ndarray, d_commands: torch.Tensor | None, scale, translate):
        """target: float32 [rows, W, 4], blended in place; vertices: 20-byte VertexP2UV2C1 records (uint8 tensor); indices: int16 or int32 tensor;
        commands: records of _lib.UI_COMMAND_DTYPE on the host, d_commands the same bytes on the device (None without commands)"""
        assert target.dtype == torch.float32 and target.shape == (self.rows, self.W, 4) and target.is_contiguous()
        assert indices.element_size() in (2, 4)
        commands = np.ascontiguousarray(commands, _lib.UI_COMMAND_DTYPE)
        assert int((commands["indexCount"] // 3).sum()) <= self.capacity, "reserve() more triangles first"
        self._scale = (C.c_float * 2)(float(scale[0]), float(scale[1]))
        self._translate = (C.c_float * 2)(float(translate[0]), float(translate[1]))
        self.ctx.call("sailor_hip_ui_draw", _ptr(vertices), vertices.numel() * vertices.element_size() // 20, _ptr(indices), indices.element_size(), indices.numel(),
                      commands.ctypes.data if len(commands) else None, _ptr(d_commands), len(commands), self._scale, self._translate, C.byref(self._texture),
                      _ptr(self.workspace), self.workspace.numel(), _ptr(target), self.W, self.H, C.byref(self.band))
        return target

    def draw_flat(self, target: torch.Tensor, flat: dict, index_bytes: int = 2):
        """host.ui_flatten's result: uploads the buffers and draws (allocates: not inside a capture)"""
        dev = self.ctx.device
        v = torch.from_numpy(np.ascontiguousarray(flat["vertices"]).view(np.uint8).copy()).to(dev)
        idx = np.ascontiguousarray(flat["indices"], np.uint32)
        i = torch.from_numpy(idx.astype(np.uint16).view(np.int16) if index_bytes == 2 else idx.view(np.int32)).to(dev)
        c = np.ascontiguousarray(flat["commands"], _lib.UI_COMMAND_DTYPE)
        dc = torch.from_numpy(c.view(np.uint8).copy()).to(dev) if len(c) else None
        self.reserve(int((c["indexCount"] // 3).sum()))
        self._buffers = (v, i, dc)
        return self.draw(target, v, i, c, dc, flat["scale"], flat["translate"])
