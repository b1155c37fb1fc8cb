"""Host-side set-up of the path: frame constants, frusta, CSM matrices, light packing, bands.

Thin numpy-facing wrappers over the `sailor_host_*` / band entry points of the C-ABI (sailor_amd/csrc/host_math.cpp,
context.hip) -- the math itself is native, mirroring what the reference does on its main/render threads before any
GPU work is recorded (FrameGraph/RHIFrameGraph.cpp:60-67, Math/Bounds.cpp:142-193, FrameGraph/ShadowPrepassNode.cpp:387-404,
ECS/LightingECS.cpp:163-172).  Nothing here needs a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Band, CsmDesc, LightCullPushConstants, UboFrameData

# ECS/LightingECS.h:71-81 / Lighting.glsl:4-15: std430 record, stride 112
LIGHT_DTYPE = np.dtype({
    "names": ["type", "shadowType", "worldPosition", "direction", "intensity", "attenuation", "cutOff", "bounds"],
    "formats": ["<u4", "<u4", ("<f4", 3), ("<f4", 3), ("<f4", 3), ("<f4", 3), ("<f4", 2), ("<f4", 3)],
    "offsets": [0, 4, 16, 32, 48, 64, 80, 96],
    "itemsize": 112,
})
# FrameGraph/RenderSceneNode.h:16-33
INSTANCE_DTYPE = np.dtype({
    "names": ["model", "sphereBounds", "materialInstance", "isCulled"],
    "formats": [("<f4", 16), ("<f4", 4), "<u4", "<u4"],
    "offsets": [0, 64, 80, 84],
    "itemsize": 96,
})

LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_SPOT, LIGHT_AREA = 0, 1, 2, 3  # Engine/Types.h:31-37
SHADOW_NONE, SHADOW_PCF, SHADOW_EVSM = 0, 1, 2                         # RHI/SceneView.h:13-18


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, n) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


def num_tiles(width: int, height: int) -> tuple[int, int]:
    tx, ty = C.c_int32(), C.c_int32()
    _lib.call("sailor_hip_num_tiles", width, height, C.byref(tx), C.byref(ty))
    return tx.value, ty.value


def band_whole_frame(width: int, height: int) -> Band:
    b = Band()
    _lib.call("sailor_hip_band_whole_frame", width, height, C.byref(b))
    return b


def band_from_tile_rows(width: int, height: int, row_begin: int, row_end: int) -> Band:
    b = Band()
    _lib.call("sailor_hip_band_from_tile_rows", width, height, row_begin, row_end, C.byref(b))
    return b


def band_for_rank(width: int, height: int, rank: int, world_size: int) -> Band:
    b = Band()
    _lib.call("sailor_hip_band_for_rank", width, height, rank, world_size, C.byref(b))
    return b


def eye_adaptation_constants(width: int, height: int, delta_time: float) -> "_lib.EyeAdaptationConstants":
    """EyeAdaptationNode.cpp:154-170: the push constants of the histogram and the average Dispatch"""
    c = _lib.EyeAdaptationConstants()
    _lib.call("sailor_host_eye_adaptation_constants", width, height, delta_time, C.byref(c))
    return c


def hbao_params(**values) -> "_lib.HbaoParams":
    """HBAO.shader:50-57 PostProcessDataUBO; unnamed members keep the shipped values (DefaultRenderer.renderer:226-230)"""
    v = dict(_lib.HBAO_SHIPPED)
    v.update(values)
    return _lib.HbaoParams(**{k: float(x) for k, x in v.items()})


def hbao_blur_params(**values) -> "_lib.HbaoBlurParams":
    """HBAO_Blur.shader:54-59 PostProcessDataUBO; unnamed members keep the shipped values (DefaultRenderer.renderer:243-245)"""
    v = dict(_lib.HBAO_BLUR_SHIPPED)
    v.update(values)
    return _lib.HbaoBlurParams(**{k: float(x) for k, x in v.items()})


def hbao_shipped_extents(width: int, height: int):
    """(HalfDepth, AO, TemporaryR8, g_AO) as (width, height): DefaultRenderer.renderer:46-72 -- ViewportWidth / 2 squared twice, ViewportWidth squared twice"""
    return (width // 2, width // 2), (width // 2, width // 2), (width, width), (width, width)


def motion_blur_params(**values) -> "_lib.MotionBlurParams":
    """MotionBlur.shader:50-55 PostProcessDataUBO; unnamed members keep the shipped values (DefaultRenderer.renderer:328-330)"""
    v = dict(_lib.MOTION_BLUR_SHIPPED)
    v.update(values)
    return _lib.MotionBlurParams(**{k: float(x) for k, x in v.items()})


def _vec4(x):
    """a scalar (the member's .x) or up to four components -> four floats"""
    c = [float(t) for t in np.atleast_1d(np.asarray(x, np.float64))]
    assert 1 <= len(c) <= 4, x
    return tuple(c + [0.0] * (4 - len(c)))


def blur_params(**values) -> "_lib.BlurParams":
    """Blur.shader:54-59 PostProcessDataUBO: blurRadius, blurCenter, blurSampleCount, each a scalar (its .x) or up to four components; unnamed members are
    zero, as in a PostProcess entry that does not set them (_lib.BLUR_GAUSS_SHIPPED / BLUR_RADIAL_SHIPPED: the shipped file's commented entries)"""
    p = _lib.BlurParams()
    for k, x in values.items():
        getattr(p, k)[:] = _vec4(x)   # (an unknown member raises AttributeError)
    return p


def chromatic_aberration_params(**values) -> "_lib.ChromaticAberrationParams":
    """ChromaticAberation.shader:52-55 PostProcessDataUBO; without `offset` it is the shipped commented entry's (DefaultRenderer.renderer:362)"""
    v = dict(_lib.CHROMATIC_ABERRATION_SHIPPED)
    v.update(values)
    p = _lib.ChromaticAberrationParams()
    for k, x in v.items():
        getattr(p, k)[:] = _vec4(x)
    return p


def bloom_params(**values) -> "_lib.BloomParams":
    """The Bloom node's four parameters; unnamed members keep the shipped values (DefaultRenderer.renderer:298-302)"""
    v = dict(_lib.BLOOM_SHIPPED)
    v.update(values)
    return _lib.BloomParams(**{k: float(x) for k, x in v.items()})


def particles_constants(num_particles: int, num_frames: int, fps: int, trace_frames: int, trace_decay: float) -> "_lib.ParticlesConstants":
    """ParticlesNode.cpp:184-189: the push constants of the update Dispatch; numInstances = n * traceFrames (:130-154)"""
    return _lib.ParticlesConstants(numInstances=int(num_particles) * int(trace_frames), numFrames=int(num_frames), fps=int(fps), traceFrames=int(trace_frames),
                                   traceDecay=float(trace_decay))


def pack_particles(enabled, size1, size2, xyz1, rgba1, xyz2, rgba2) -> np.ndarray:
    """arrays over the records -> SailorParticleData records (_lib.PARTICLE_DATA_DTYPE, 80 bytes each); the two unused words are 0"""
    n = len(np.atleast_1d(enabled))
    r = np.zeros(n, dtype=_lib.PARTICLE_DATA_DTYPE)
    r["enabled"], r["size1"], r["size2"] = enabled, size1, size2
    r["xyz1"], r["rgba1"] = np.asarray(xyz1, np.float32).reshape(n, 3), np.asarray(rgba1, np.float32).reshape(n, 4)
    r["xyz2"], r["rgba2"] = np.asarray(xyz2, np.float32).reshape(n, 3), np.asarray(rgba2, np.float32).reshape(n, 4)
    return r


def particle_instances(records: np.ndarray, num_particles: int, trace_frames: int, material_instance: int = 0) -> np.ndarray:
    """ParticlesNode.cpp:130-152: the instance buffer as the node builds it once on the host (_lib.PARTICLE_INSTANCE_DTYPE): instance i belongs to particle
    i // traceFrames; model = translate(x2, y2, z2) * scale(size2), color = 1, colorOld = 0, materialInstance set"""
    n = int(num_particles) * int(trace_frames)
    inst = np.zeros(n, dtype=_lib.PARTICLE_INSTANCE_DTYPE)
    j = np.arange(n) // int(trace_frames)
    m = np.zeros((n, 4, 4), np.float32)  # [column][row]
    s = records["size2"][j]
    m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = s
    m[:, 3, :3] = records["xyz2"][j]
    m[:, 3, 3] = 1.0
    inst["model"] = m.reshape(n, 16)
    inst["color"] = 1.0
    inst["materialInstance"] = material_instance
    return inst


def bloom_push_constants(threshold: float, knee: float) -> np.ndarray:
    """BloomNode.cpp:89-93: u_threshold = (t, t - knee, 2 knee, 0.25 knee) as float32[4]"""
    out = np.empty(4, np.float32)
    _lib.call("sailor_host_bloom_push_constants", threshold, knee, _fp(out))
    return out


def mip_chain_extents(width: int, height: int, levels: int):
    """[(width, height)] of the levels of a mip chain: max(1, dim >> level)"""
    return [(max(1, width >> l), max(1, height >> l)) for l in range(levels)]


def mip_chain_texels(width: int, height: int, levels: int) -> int:
    """texels of the first `levels` levels of a level-major chain = the texel offset of level `levels` (sailor_hip_mip_chain_texels)"""
    return int(_lib.load().sailor_hip_mip_chain_texels(width, height, levels))


def sky_params(**overrides) -> "_lib.SkyParams":
    """SkyNode::SkyParams with the initialisers of SkyNode.h:50-67; `lightDirection` takes 3 or 4 floats (w = 0), the other members by name"""
    p = _lib.SkyParams()
    _lib.call("sailor_host_sky_params_default", C.byref(p))
    for name, value in overrides.items():
        if name == "lightDirection":
            v = [float(x) for x in value]
            p.lightDirection[:] = (v + [0.0])[:4] if len(v) == 3 else v
        elif name in ("scatteringSteps", "sunShaftsDistance"):
            setattr(p, name, int(value))
        elif name in dict(_lib.SkyParams._fields_):
            setattr(p, name, float(value))
        else:
            raise ValueError(f"SkyParams has no member {name!r}")
    return p


def sky_sun_color(sun_direction) -> np.ndarray:
    """Sky.shader:247-264 CalculateSunColor(sunDirection) in fp32; the cloud march passes -dirToSun"""
    d, out = _f32(sun_direction, 3), np.empty(3, np.float32)
    _lib.call("sailor_host_sky_sun_color", _fp(d), _fp(out))
    return out


def sky_star_color_table(rows) -> np.ndarray:
    """SkyNode.cpp:47-58: the `colors` rows of StarsColor.yaml ([n, 11] floats) -> the node's temperature table, float32 [391, 3]"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert rows.ndim == 2 and rows.shape[1] == 11, rows.shape
    out = np.empty((_lib.SKY_STAR_TABLE_ROWS, 3), np.float32)
    _lib.call("sailor_host_sky_star_color_table", _fp(rows), rows.shape[0], _fp(out))
    return out


def sky_star_mesh(catalogue: bytes, table):
    """SkyNode.cpp:61-91: the BSC5 bytes and the temperature table -> (positions float32 [n, 3], colours float32 [n, 4]); a truncated catalogue raises"""
    table = _f32(table, _lib.SKY_STAR_TABLE_ROWS * 3)
    data = bytes(catalogue)
    capacity = max(0, len(data) - 28) // 32
    pos, col, count = np.empty((capacity, 3), np.float32), np.empty((capacity, 4), np.float32), C.c_uint32()
    _lib.call("sailor_host_sky_star_mesh", data, len(data), _fp(table), _fp(pos), _fp(col), capacity, C.byref(count))
    return pos[:count.value].copy(), col[:count.value].copy()


def sky_stars_model(camera_position) -> np.ndarray:
    """SkyNode.cpp:208-211, :698: translate(cameraPosition) * toMat4(precession), column-major float32[16]"""
    cam, out = np.ascontiguousarray(camera_position, dtype=np.float32).reshape(-1)[:3].copy(), np.empty(16, np.float32)
    _lib.call("sailor_host_sky_stars_model", _fp(cam), _fp(out))
    return out


def sky_face_matrices(face: int):
    """SkyNode.cpp:487-508: (view, projection, invProjection) of cube face 0..5, column-major float32[16] each"""
    v, p, ip = (np.empty(16, np.float32) for _ in range(3))
    _lib.call("sailor_host_sky_face_matrices", face, _fp(v), _fp(p), _fp(ip))
    return v, p, ip


def transform_matrix(position, rotation_xyzw, scale) -> np.ndarray:
    """Math/Transform.cpp:39-42; returns a column-major float32[16]."""
    trs = np.concatenate([_f32(position, 4), _f32(rotation_xyzw, 4), _f32(scale, 4)])
    out = np.empty(16, np.float32)
    _lib.call("sailor_host_transform_matrix", _fp(trs), _fp(out))
    return out


def mat4_inverse(m) -> np.ndarray:
    m = _f32(m, 16)
    out = np.empty(16, np.float32)
    _lib.call("sailor_host_mat4_inverse", _fp(m), _fp(out))
    return out


def mat4_mul(a, b) -> np.ndarray:
    a, b = _f32(a, 16), _f32(b, 16)
    out = np.empty(16, np.float32)
    _lib.call("sailor_host_mat4_mul", _fp(a), _fp(b), _fp(out))
    return out


def fill_frame_data(camera_world, fov_degrees: float, z_near: float, z_far: float, width: int, height: int,
                    current_time: float = 0.0, delta_time: float = 0.0, aspect: float | None = None) -> UboFrameData:
    """FrameGraph/RHIFrameGraph.cpp:60-67 (+ ECS/CameraECS.cpp:20,33, Math/Math.cpp:18-21)."""
    cw = _f32(camera_world, 16)
    frame = UboFrameData()
    asp = np.float32(width) / np.float32(height) if aspect is None else np.float32(aspect)
    _lib.call("sailor_host_fill_frame_data", _fp(cw), fov_degrees, float(asp), z_near, z_far, width, height, current_time, delta_time, C.byref(frame))
    return frame


def push_constants(frame: UboFrameData, width: int, height: int, lights_num: int) -> LightCullPushConstants:
    """FrameGraph/LightCullingNode.cpp:51-57."""
    pc = LightCullPushConstants()
    pc.viewportSize[0], pc.viewportSize[1] = width, height
    tx, ty = num_tiles(width, height)
    pc.numTiles[0], pc.numTiles[1] = tx, ty
    pc.lightsNum = lights_num
    return pc


def extract_frustum_planes(world_matrix, aspect: float, fov_y_degrees: float, z_near: float, z_far: float):
    """Math/Bounds.cpp:142-193 -> (planes float32[6,4] in L,R,T,B,N,F order, corners float32[8,3])."""
    wm = _f32(world_matrix, 16)
    planes = np.empty(24, np.float32)
    corners = np.empty(24, np.float32)
    _lib.call("sailor_host_extract_frustum_planes", _fp(wm), aspect, fov_y_degrees, z_near, z_far, _fp(planes), _fp(corners))
    return planes.reshape(6, 4), corners.reshape(8, 3)


def extract_frustum_planes_matrix(projection_view_matrix):
    """Math/Bounds.cpp:20-67 Frustum::ExtractFrustumPlanes(projectionViewMatrix) -> (planes float32[6,4] L,R,T,B,N,F, corners float32[8,3])."""
    m = _f32(projection_view_matrix, 16)
    planes = np.empty(24, np.float32)
    corners = np.empty(24, np.float32)
    _lib.call("sailor_host_extract_frustum_planes_matrix", _fp(m), _fp(planes), _fp(corners))
    return planes.reshape(6, 4), corners.reshape(8, 3)


def quat_rotate(q_xyzw, v) -> np.ndarray:
    """glm::rotate(quat, vec3) = v + ((cross(q.xyz, v) * q.w) + cross(q.xyz, cross(q.xyz, v))) * 2, in float32 (Math/Transform.cpp:74 GetForward)"""
    q = np.asarray(q_xyzw, np.float32)
    v = np.asarray(v, np.float32)
    uv = np.cross(q[:3], v).astype(np.float32)
    uuv = np.cross(q[:3], uv).astype(np.float32)
    return (v + (uv * q[3] + uuv) * np.float32(2.0)).astype(np.float32)


CSM_CAMERA_POS_DELTA = np.float32(15.0)        # ECS/LightingECS.cpp:16
CSM_CAMERA_ROTATION_DELTA = np.float32(0.9995)  # ECS/LightingECS.cpp:17


def csm_view_unchanged(prev_view, view) -> bool:
    """The transform half of CSMLightState::Equals (ECS/LightingECS.cpp:14-24).  A view is (component index, camera position[4], camera rotation xyzw,
    light position[4], light rotation xyzw): unchanged iff same light component, the camera moved at most 15 units and its forward vector keeps a
    dot product of at least 0.9995 with the old one, and the light's position and rotation are exactly equal."""
    if prev_view is None or view is None:
        return prev_view is None and view is None
    (ci0, cp0, cr0, lp0, lr0), (ci1, cp1, cr1, lp1, lr1) = prev_view, view
    if ci0 != ci1:
        return False
    d = np.asarray(cp0, np.float32) - np.asarray(cp1, np.float32)
    if np.sqrt(np.float32(np.dot(d, d)), dtype=np.float32) > CSM_CAMERA_POS_DELTA:
        return False
    f0, f1 = quat_rotate(cr0, [0, 0, -1]), quat_rotate(cr1, [0, 0, -1])
    if np.float32(np.dot(f0, f1)) < CSM_CAMERA_ROTATION_DELTA:
        return False
    return bool(np.array_equal(np.asarray(lp0, np.float32), np.asarray(lp1, np.float32)) and np.array_equal(np.asarray(lr0, np.float32), np.asarray(lr1, np.float32)))


class CsmSnapshots:
    """LightingECS::m_csmSnapshots behind the C-ABI (sailor_host_csm_snapshots_*): `snaps[k]` = (mesh indices, their last-changed frames, the view the
    snapshot was taken with or None)."""

    def __init__(self, handle=None):
        lib = _lib.load()
        self._lib = lib
        self.handle = handle if handle is not None else lib.sailor_host_csm_snapshots_create()
        if not self.handle:
            raise MemoryError("sailor_host_csm_snapshots_create")

    def clone(self) -> "CsmSnapshots":
        return CsmSnapshots(self._lib.sailor_host_csm_snapshots_clone(self.handle))

    def __len__(self):
        return int(self._lib.sailor_host_csm_snapshots_count(self.handle))

    def __getitem__(self, k: int):
        n = C.c_uint32()
        _lib.call("sailor_host_csm_snapshot_get", self.handle, k, 0, C.byref(n), None, None, None, None)
        idx = np.zeros(max(n.value, 1), np.uint32); frames = np.zeros(max(n.value, 1), np.uint64)
        has = C.c_int32(); v = _lib.CsmView()
        _lib.call("sailor_host_csm_snapshot_get", self.handle, k, n.value, C.byref(n), idx.ctypes.data_as(C.c_void_p), frames.ctypes.data_as(C.c_void_p), C.byref(has),
                  C.byref(v))
        view = (int(v.componentIndex), np.float32(list(v.cameraPosition)), np.float32(list(v.cameraRotation)), np.float32(list(v.lightPosition)),
                np.float32(list(v.lightRotation))) if has.value else None
        return idx[: n.value], frames[: n.value], view

    def __del__(self):
        try:
            if self.handle:
                self._lib.sailor_host_csm_snapshots_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def _csm_view_struct(view):
    v = _lib.CsmView()
    v.componentIndex = int(view[0])
    for name, vals in zip(("cameraPosition", "cameraRotation", "lightPosition", "lightRotation"), view[1:]):
        a = np.asarray(vals, np.float32)
        for i in range(4):
            getattr(v, name)[i] = float(a[i])
    return v


def plan_csm_passes(overlap_masks: np.ndarray, shadow_types, last_changed_frame: np.ndarray, previous, view=None):
    """The bookkeeping of LightingECS::PrepareCSMPasses (ECS/LightingECS.cpp:299-366) for one directional light -- sailor_host_csm_plan_passes
    (host_math.cpp) -- on the cascade overlap sets of sailor_hip_csm_caster_masks (uint64 [cascades, words]):
      * cascade k > 0 drops every mesh that an EARLIER cascade of the same shadow type, re-rendered this frame, already overlaps (:310-327);
      * a cascade is re-rendered iff its mesh list, as (mesh index, frame the mesh last changed) pairs, differs from last frame's snapshot
        or -- with `view` = (light component index, camera position, camera rotation, light position, light rotation) -- the camera moved more than 15
        units / turned past dot 0.9995 / the light moved at all since that snapshot was taken (CSMLightState::Equals :14-38, csm_view_unchanged).
        A cascade that is NOT re-rendered keeps its old snapshot, camera included (:353-357): slow camera drift accumulates until it crosses the threshold.
    `previous`: the CsmSnapshots a former call returned, or None.  Returns (list of cascades to render, their final uint64 masks [cascades, words],
    the new CsmSnapshots; `previous` is left as it was)."""
    masks_in = np.ascontiguousarray(overlap_masks, np.uint64)
    n_casc, words = masks_in.shape
    frames = np.ascontiguousarray(last_changed_frame, np.uint64)
    n = len(frames)
    assert words == (n + 63) // 64
    types = np.ascontiguousarray(shadow_types, np.uint32)
    snaps = previous.clone() if previous is not None else CsmSnapshots()
    render = np.zeros(n_casc, np.uint32)
    out = np.zeros_like(masks_in)
    vs = _csm_view_struct(view) if view is not None else None
    _lib.call("sailor_host_csm_plan_passes", snaps.handle, 0, n_casc, n, masks_in.ctypes.data_as(C.c_void_p), types.ctypes.data_as(C.c_void_p),
              frames.ctypes.data_as(C.c_void_p), C.byref(vs) if vs is not None else None, render.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return [int(k) for k in np.nonzero(render)[0]], out, snaps


def overlaps_sphere(planes, center, radius: float) -> bool:
    """Math/Bounds.cpp:211-226 Frustum::OverlapsSphere"""
    pl = _f32(planes, 24); sp = np.float32([center[0], center[1], center[2], radius])
    return bool(_lib.load().sailor_host_overlaps_sphere(_fp(pl), _fp(sp)))


def contains_sphere(planes, center, radius: float) -> bool:
    """Math/Bounds.cpp:228-243 Frustum::ContainsSphere"""
    pl = _f32(planes, 24); sp = np.float32([center[0], center[1], center[2], radius])
    return bool(_lib.load().sailor_host_contains_sphere(_fp(pl), _fp(sp)))


def lights_in_frustum(planes, camera_position, types, shadow_types, positions, bounds, active=None):
    """LightingECS::GetLightsInFrustum (ECS/LightingECS.cpp:209-260) -> (directional indices, (point indices, distances), (spot indices, distances))"""
    n = len(types)
    pl = _f32(planes, 24); cp = np.float32(camera_position)[:3].copy()
    t = np.ascontiguousarray(types, np.uint32); st = np.ascontiguousarray(shadow_types, np.uint32)
    pos = np.ascontiguousarray(positions, np.float32).reshape(n, 3); bd = np.ascontiguousarray(bounds, np.float32).reshape(n, 3)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    od, op, os_ = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
    dp, ds = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    nd, npt, ns = C.c_uint32(), C.c_uint32(), C.c_uint32()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _lib.call("sailor_host_lights_in_frustum", _fp(pl), _fp(cp), n, vp(t), vp(st), vp(act), vp(pos), vp(bd), vp(od), C.byref(nd), vp(op), vp(dp), C.byref(npt), vp(os_),
              vp(ds), C.byref(ns))
    return od[: nd.value].copy(), (op[: npt.value].copy(), dp[: npt.value].copy()), (os_[: ns.value].copy(), ds[: ns.value].copy())


def csm_matrices(light_view, camera_world, aspect: float, fov_y_degrees: float, camera_near: float, camera_far: float) -> np.ndarray:
    """The 4 `lightsMatrices` (FrameGraph/ShadowPrepassNode.cpp:387-404, ECS/LightingECS.cpp:292) as float32[4,16]."""
    lv, cw = _f32(light_view, 16), _f32(camera_world, 16)
    out = np.empty(64, np.float32)
    _lib.call("sailor_host_csm_matrices", _fp(lv), _fp(cw), aspect, fov_y_degrees, camera_near, camera_far, _fp(out))
    return out.reshape(4, 16)


def cutoff_cosines(inner_degrees: float, outer_degrees: float) -> tuple[np.float32, np.float32]:
    """ECS/LightingECS.cpp:171 through the native packer."""
    z3 = np.zeros(3, np.float32)
    cut = np.array([inner_degrees, outer_degrees], np.float32)
    rec = _lib.LightShaderData()
    _lib.call("sailor_host_pack_light", 1, 0, _fp(z3), _fp(z3), _fp(z3), _fp(z3), _fp(cut), _fp(z3), C.byref(rec))
    return np.float32(rec.cutOff[0]), np.float32(rec.cutOff[1])


def make_csm_desc(lights_matrices: np.ndarray, maps: list) -> CsmDesc:
    """maps: list of 4 (device_ptr | 0, width, height, format)."""
    d = CsmDesc()
    lm = np.ascontiguousarray(lights_matrices, np.float32).reshape(4, 16)
    for k in range(4):
        for i in range(16):
            d.lightsMatrices[k][i] = float(lm[k, i])
        ptr, w, h, fmt = maps[k]
        d.maps[k] = ptr or None
        d.width[k], d.height[k], d.format[k] = w, h, fmt
    return d


def srgb_table() -> np.ndarray:
    """sailor_host_srgb_table: the sRGB transfer function of the 256 byte values (double, rounded once to fp32)"""
    out = np.zeros(256, np.float32)
    _lib.call("sailor_host_srgb_table", _fp(out))
    return out


def srgb_encode_table() -> np.ndarray:
    """sailor_host_srgb_encode_table: the 255 rounding boundaries of the sRGB encode, out[k - 1] = the decode of (k - 0.5) / 255 (double, rounded once to fp32);
    the byte of x is the number of entries <= x"""
    out = np.zeros(255, np.float32)
    _lib.call("sailor_host_srgb_encode_table", _fp(out))
    return out


def texture_mip_levels(width: int, height: int) -> int:
    """sailor_hip_texture_mip_levels: floor(log2(max(width, height))) + 1, 0 for an extent outside 1 .. 32768"""
    return int(_lib.load().sailor_hip_texture_mip_levels(width, height))


def msaa_sample_positions(samples: int) -> np.ndarray:
    """sailor_host_msaa_sample_positions: the standard sample locations of a `samples`-times multisampled pixel, int32 [samples, 2], (sx, sy) in 1/256 pixel
    from the pixel's top-left corner; samples is 1, 2, 4 or 8"""
    out = np.zeros((max(int(samples), 1), 2), np.int32)
    _lib.call("sailor_host_msaa_sample_positions", samples, out.ctypes.data_as(C.c_void_p))
    return out


def surface_draw_prims(num_triangles: int, num_drawn: int) -> int:
    """sailor_hip_surface_draw_prims: what a draw adds to the surface pass's running primBase"""
    out = C.c_uint64()
    _lib.call("sailor_hip_surface_draw_prims", num_triangles, num_drawn, C.byref(out))
    return int(out.value)


def debug_lines_prims(num_segments: int) -> int:
    """sailor_hip_debug_lines_prims: what the DebugDraw pass's draw adds to a running primBase"""
    out = C.c_uint64()
    _lib.call("sailor_hip_debug_lines_prims", num_segments, C.byref(out))
    return int(out.value)


# ---- RHI/DebugContext.cpp: the line lists of the debug shapes, in the reference's segment order and fp32 arithmetic.  Each returns VertexP3C4 records
# (_lib.VERTEX_P3C4_DTYPE), two per segment: what DrawLine (:76-98) appends. -------------------------------------------------------------------------
def _v3(v) -> np.ndarray:
    return np.asarray(v, np.float32).reshape(3)


def debug_line(start, end, color) -> np.ndarray:
    """DebugContext::DrawLine (:76-98): both vertices get the colour"""
    out = np.zeros(2, _lib.VERTEX_P3C4_DTYPE)
    out["position"][0], out["position"][1] = _v3(start), _v3(end)
    out["color"][:] = np.asarray(color, np.float32).reshape(4)
    return out


def _debug_lines(pairs, color) -> np.ndarray:
    return np.concatenate([debug_line(a, b, c if c is not None else color) for a, b, *rest in pairs for c in [rest[0] if rest else None]])


def debug_aabb(aabb_min, aabb_max, color) -> np.ndarray:
    """DebugContext::DrawAABB (:100-116): 12 segments"""
    a, b = _v3(aabb_min), _v3(aabb_max)
    v = lambda x, y, z: np.array([x[0], y[1], z[2]], np.float32)  # noqa: E731
    return _debug_lines([(a, v(b, a, a)), (a, v(a, b, a)), (a, v(a, a, b)),
                         (b, v(a, b, b)), (b, v(b, a, b)), (b, v(b, b, a)),
                         (v(a, b, b), v(a, b, a)), (v(a, b, b), v(a, a, b)), (v(a, a, b), v(b, a, b)),
                         (v(b, a, b), v(b, a, a)), (v(b, a, a), v(b, b, a)), (v(b, b, a), v(a, b, a))], color)


def debug_frustum(corners, color) -> np.ndarray:
    """DebugContext::DrawFrustum (:140-158) over Frustum::GetCorners() (extract_frustum_planes' second result): 12 segments, the second four white"""
    c = np.asarray(corners, np.float32).reshape(8, 3)
    white = (1.0, 1.0, 1.0, 1.0)
    return _debug_lines([(c[4], c[5]), (c[5], c[6]), (c[6], c[7]), (c[7], c[4]),
                         (c[0], c[1], white), (c[1], c[2], white), (c[2], c[3], white), (c[3], c[0], white),
                         (c[4], c[0]), (c[5], c[1]), (c[6], c[2]), (c[7], c[3])], color)


def debug_origin(position, origin, size: float) -> np.ndarray:
    """DebugContext::DrawOrigin (:129-138): origin * vec4(size, 0, 0, 0) etc. as glm's mat4 * vec4, (c0 x + c1 y) + (c2 z + c3 w), from `position`; red, green, blue"""
    p, m, s = _v3(position), np.asarray(origin, np.float32).reshape(4, 4), np.float32(size)  # m[c] = column c
    z = np.float32(0.0)
    axis = lambda x, y, w: ((m[0] * x + m[1] * y) + (m[2] * w + m[3] * z))[:3]  # noqa: E731
    return _debug_lines([(p, p + axis(s, z, z), (1, 0, 0, 1)), (p, p + axis(z, s, z), (0, 1, 0, 1)), (p, p + axis(z, z, s), (0, 0, 1, 1))], None)


def debug_arrow(start, end, color) -> np.ndarray:
    """DebugContext::DrawArrow (:118-127): the segment and a three-axis cross of a tenth of its length at the end"""
    a, b = _v3(start), _v3(end)
    d = b - a
    length = np.float32(np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))) * np.float32(0.1)
    up, left, forward = np.array([0, 1, 0], np.float32), np.array([-1, 0, 0], np.float32), np.array([0, 0, -1], np.float32)
    return _debug_lines([(a, b), (b + up * length, b + (-up) * length), (b + left * length, b + (-left) * length),
                         (b + forward * length, b + (-forward) * length)], color)


def debug_sphere(position, radius: float, color) -> np.ndarray:
    """DebugContext::DrawSphere (:17-63) in fp32 with its (i - 1) / (j - 1) indexing: 8 latitude bands x (1 + 7 x 3) = 176 segments"""
    p, r, pi, n = _v3(position), np.float32(radius), np.float32(3.1415926), 7  # Math::Pi (Math.h:14)
    pairs = []
    for i in range(n + 1):
        lat0 = pi * (np.float32(-0.5) + np.float32(i - 1) / np.float32(n))
        lat1 = pi * (np.float32(-0.5) + np.float32(i) / np.float32(n))
        z0, zr0, z1, zr1 = np.sin(lat0), np.cos(lat0), np.sin(lat1), np.cos(lat1)
        v3 = v4 = None
        for j in range(n + 1):
            lng = np.float32(2) * pi * np.float32(j - 1) / np.float32(n)
            x, y = np.cos(lng), np.sin(lng)
            v1 = p + np.array([r * x * zr0, r * z0, r * y * zr0], np.float32)
            v2 = p + np.array([r * x * zr1, r * z1, r * y * zr1], np.float32)
            if v3 is not None:
                pairs += [(v1, v3), (v2, v4)]
            pairs.append((v1, v2))
            v3, v4 = v1, v2
    return _debug_lines(pairs, color)


# ---- Submodules/ImGuiApi.cpp: draw data for the RenderImGui pass as plain data, and small draw-list builders for callers without ImGui.  Draw data is a dict:
# display_pos, display_size, framebuffer_scale (pairs) and lists; a list is a dict of vertices (records of _lib.VERTEX_P2UV2C1_DTYPE), indices (unsigned) and
# cmds; a command is a dict of clip_rect (x1, y1, x2, y2), elem_count, idx_offset, vtx_offset and callback (_lib.UI_CALLBACK_*). ---------------------------------
def ui_color(r: float, g: float, b: float, a: float) -> int:
    """IM_COL32 from floats in [0, 1]: r in the low byte"""
    q = [int(round(min(max(float(c), 0.0), 1.0) * 255.0)) for c in (r, g, b, a)]
    return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24)


def ui_flatten(draw_data: dict) -> dict:
    """sailor_host_ui_flatten: -> width, height, scale, translate (the push constants), commands (records of _lib.UI_COMMAND_DTYPE; skipped commands left
    out), and the merged vertices and indices in list order (ImGui_UpdateDrawData :170-185)"""
    lists = draw_data.get("lists", [])
    cl = (_lib.UiDrawList * max(len(lists), 1))()
    flat = [c for l in lists for c in l["cmds"]]
    cc = (_lib.UiDrawCmd * max(len(flat), 1))()
    first = 0
    for n, l in enumerate(lists):
        cl[n] = _lib.UiDrawList(len(l["vertices"]), len(l["indices"]), first, len(l["cmds"]))
        first += len(l["cmds"])
    for n, c in enumerate(flat):
        cc[n] = _lib.UiDrawCmd((C.c_float * 4)(*[float(x) for x in c["clip_rect"]]), int(c.get("elem_count", 0)), int(c.get("idx_offset", 0)),
                               int(c.get("vtx_offset", 0)), int(c.get("callback", _lib.UI_CALLBACK_NONE)))
    f2 = lambda v: (C.c_float * 2)(*[float(x) for x in v])  # noqa: E731
    pc, count, w, h = (C.c_float * 4)(), C.c_uint32(), C.c_int32(), C.c_int32()
    out = (_lib.UiCommand * max(len(flat), 1))()
    _lib.call("sailor_host_ui_flatten", f2(draw_data["display_pos"]), f2(draw_data["display_size"]), f2(draw_data["framebuffer_scale"]), cl, len(lists), cc, len(flat),
              pc, out, len(flat), C.byref(count), C.byref(w), C.byref(h))
    commands = np.frombuffer(bytes(out), _lib.UI_COMMAND_DTYPE)[: count.value].copy()
    vertices = np.concatenate([np.asarray(l["vertices"], _lib.VERTEX_P2UV2C1_DTYPE) for l in lists]) if lists else np.zeros(0, _lib.VERTEX_P2UV2C1_DTYPE)
    indices = np.concatenate([np.asarray(l["indices"], np.uint32) for l in lists]) if lists else np.zeros(0, np.uint32)
    return dict(width=int(w.value), height=int(h.value), scale=np.float32([pc[0], pc[1]]), translate=np.float32([pc[2], pc[3]]), commands=commands,
                vertices=vertices, indices=indices)


class UiDrawList:
    """An ImDrawList as far as the pass reads it: vertices, indices and commands.  clip() opens a command (as PushClipRect does), the shape calls append to
    the open one.  white_uv: the atlas texel ImGui keeps white for untextured shapes (ImFontAtlas::TexUvWhitePixel)."""

    def __init__(self, white_uv=(0.0, 0.0)):
        self.white_uv, self._v, self._i, self.cmds = white_uv, [], [], []

    def clip(self, x1: float, y1: float, x2: float, y2: float):
        self.cmds.append(dict(clip_rect=(x1, y1, x2, y2), elem_count=0, idx_offset=len(self._i), vtx_offset=0, callback=_lib.UI_CALLBACK_NONE))
        return self

    def callback(self, kind: int):
        """AddCallback: a command that draws nothing; the next shape needs a clip() of its own"""
        self.cmds.append(dict(clip_rect=(0.0, 0.0, 0.0, 0.0), elem_count=0, idx_offset=len(self._i), vtx_offset=0, callback=kind))
        return self

    def _add(self, verts, idx):
        assert self.cmds and self.cmds[-1]["callback"] == _lib.UI_CALLBACK_NONE, "open a command with clip() first"
        base = len(self._v)
        self._v += verts
        self._i += [base + k for k in idx]
        self.cmds[-1]["elem_count"] += len(idx)
        return self

    def quad(self, x0, y0, x1, y1, uv0, uv1, color: int):
        """PrimRectUV: a, b, c and a, c, d over the corners (x0, y0), (x1, y0), (x1, y1), (x0, y1) -- a glyph quad when uv spans a glyph's cell"""
        return self._add([((x0, y0), (uv0[0], uv0[1]), color), ((x1, y0), (uv1[0], uv0[1]), color), ((x1, y1), (uv1[0], uv1[1]), color),
                          ((x0, y1), (uv0[0], uv1[1]), color)], [0, 1, 2, 0, 2, 3])

    def rect(self, x0, y0, x1, y1, color: int):
        """PrimRect: a filled rect, two triangles, every vertex at the white pixel"""
        return self.quad(x0, y0, x1, y1, self.white_uv, self.white_uv, color)

    def triangle(self, p0, p1, p2, colors, uvs=None):
        uvs = uvs or [self.white_uv] * 3
        c = colors if isinstance(colors, (list, tuple)) else [colors] * 3
        return self._add([(tuple(p0), tuple(uvs[0]), c[0]), (tuple(p1), tuple(uvs[1]), c[1]), (tuple(p2), tuple(uvs[2]), c[2])], [0, 1, 2])

    def rect_aa(self, x0, y0, x1, y1, color: int, fringe: float = 1.0):
        """AddConvexPolyFilled with anti-aliasing over a rect: the inner rect in `color` and, round it, a fringe of thin triangles whose outer vertices
        have alpha 0 (inner ring pulled in by half the fringe, outer ring pushed out by half)"""
        h, clear = 0.5 * fringe, color & 0x00FFFFFF
        inner = [(x0 + h, y0 + h), (x1 - h, y0 + h), (x1 - h, y1 - h), (x0 + h, y1 - h)]
        outer = [(x0 - h, y0 - h), (x1 + h, y0 - h), (x1 + h, y1 + h), (x0 - h, y1 + h)]
        verts = [(p, self.white_uv, color) for p in inner] + [(p, self.white_uv, clear) for p in outer]
        idx = [0, 1, 2, 0, 2, 3]
        for k in range(4):
            n = (k + 1) % 4
            idx += [k, 4 + k, 4 + n, k, 4 + n, n]
        return self._add(verts, idx)

    def data(self) -> dict:
        v = np.zeros(len(self._v), _lib.VERTEX_P2UV2C1_DTYPE)
        for k, (p, uv, c) in enumerate(self._v):
            v["position"][k], v["uv"][k], v["color"][k] = p, uv, c
        return dict(vertices=v, indices=np.asarray(self._i, np.uint32), cmds=[dict(c) for c in self.cmds])


def ui_draw_data(lists, display_size, display_pos=(0.0, 0.0), framebuffer_scale=(1.0, 1.0)) -> dict:
    """ImDrawData over UiDrawList builders or list dicts"""
    return dict(display_pos=tuple(display_pos), display_size=tuple(display_size), framebuffer_scale=tuple(framebuffer_scale),
                lists=[l.data() if isinstance(l, UiDrawList) else l for l in lists])
