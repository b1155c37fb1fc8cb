"""ctypes binding of the C-ABI declared in include/sailor_hip.h (libsailor_hip.so).

This is the same binding a maintainer of the reference would write for its HIP backend;
the Python layer above it only does plumbing: device memory and streams come from torch, the arithmetic is in the
hand-written HIP kernels behind these entry points.  There is no CPU fallback: if the shared library is missing,
or a device entry point reports an error, a SailorHipError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = _CSRC / "libsailor_hip.so"

TILE = 16            # Constants.glsl:13
CANDIDATES = 196     # Constants.glsl:14
LIGHTS_PER_TILE = 128  # Constants.glsl:15
NUM_CASCADES = 4     # Constants.glsl:23

CTX_OWN_STREAM = 1
CULL_DEFAULT = 0
CULL_BRUTE_FORCE = 1
CULL_RAW_DEPTH = 2
CULL_INTERVAL_MASKS = 4
CULL_DEFER_PACK = 8
CULL_PREPARE_LIGHTS = 16
CULL_BAND_SELECT = 32
CULL_NO_BAND_SELECT = 64
CULL_PREPARE_SELECTED = 128

RASTER_CLEAR, RASTER_CULL_BACK = 1, 2
SHADOWMAP_R16F = 0
SHADOWMAP_RGBA32F = 1
SHADOWMAP_R32F = 2

TONEMAP_ACES, TONEMAP_UNCHARTED2, TONEMAP_LUMINANCE = 1, 2, 4  # Tonemapping.shader:6-9 defines
TONEMAP_DEFINES = {"ACES": TONEMAP_ACES, "UNCHARTED2": TONEMAP_UNCHARTED2, "LUMINANCE": TONEMAP_LUMINANCE}

TRACE_FLAT_FLOAT_BOXES = 0    # the float world boxes, tested flat (sailor_hip_ecs_sweep)
TRACE_OCTREE_INT_BOXES = 1    # RHISceneView::TraceScene as the reference runs it: integer boxes in a TOctree
OCTREE_ROOT_SIZE = 16536 * 16  # RHI/SceneView.h:91-92
TRACE_MODES = {"flat": TRACE_FLAT_FLOAT_BOXES, "octree": TRACE_OCTREE_INT_BOXES}


class SailorHipError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status} ({status_string(status)}) {detail}".rstrip())


class UboFrameData(C.Structure):  # RHI/Types.h:751-761
    _fields_ = [("view", C.c_float * 16), ("projection", C.c_float * 16), ("invProjection", C.c_float * 16),
                ("cameraPosition", C.c_float * 4), ("viewportSize", C.c_int32 * 2), ("cameraZNearZFar", C.c_float * 2),
                ("currentTime", C.c_float), ("deltaTime", C.c_float)]


class LightCullPushConstants(C.Structure):  # FrameGraph/LightCullingNode.h:25-31
    _fields_ = [("invViewProjection", C.c_float * 16), ("viewportSize", C.c_int32 * 2), ("numTiles", C.c_int32 * 2),
                ("lightsNum", C.c_int32), ("_pad", C.c_int32)]


class LightShaderData(C.Structure):  # ECS/LightingECS.h:71-81
    _fields_ = [("type", C.c_uint32), ("shadowType", C.c_uint32), ("_pad0", C.c_uint32 * 2),
                ("worldPosition", C.c_float * 3), ("_pad1", C.c_float),
                ("direction", C.c_float * 3), ("_pad2", C.c_float),
                ("intensity", C.c_float * 3), ("_pad3", C.c_float),
                ("attenuation", C.c_float * 3), ("_pad4", C.c_float),
                ("cutOff", C.c_float * 2), ("_pad5", C.c_float * 2),
                ("bounds", C.c_float * 3), ("_pad6", C.c_float)]


class Band(C.Structure):
    _fields_ = [("tileRowBegin", C.c_int32), ("tileRowEnd", C.c_int32), ("fbRowBegin", C.c_int32), ("fbRowCount", C.c_int32)]

    def __repr__(self):
        return f"Band(tileRows=[{self.tileRowBegin},{self.tileRowEnd}), fbRows=[{self.fbRowBegin},{self.fbRowBegin + self.fbRowCount}))"


class CsmDesc(C.Structure):
    _fields_ = [("lightsMatrices", (C.c_float * 16) * NUM_CASCADES), ("maps", C.c_void_p * NUM_CASCADES),
                ("width", C.c_int32 * NUM_CASCADES), ("height", C.c_int32 * NUM_CASCADES), ("format", C.c_int32 * NUM_CASCADES)]


class CsmView(C.Structure):  # include/sailor_hip.h SailorCsmView (the transform half of CSMLightState, ECS/LightingECS.cpp:14-38)
    _fields_ = [("componentIndex", C.c_uint32), ("cameraPosition", C.c_float * 4), ("cameraRotation", C.c_float * 4),
                ("lightPosition", C.c_float * 4), ("lightRotation", C.c_float * 4)]


class SceneTrace(C.Structure):  # include/sailor_hip.h SailorSceneTrace
    _fields_ = [("mode", C.c_uint32), ("rootSize", C.c_uint32), ("dInserted", C.c_void_p)]


class ShadowGatherJob(C.Structure):  # include/sailor_hip.h SailorShadowGatherJob
    _fields_ = [("dMask", C.c_void_p), ("begin", C.c_uint32), ("end", C.c_uint32), ("dOut", C.c_void_p), ("capacity", C.c_uint32), ("_pad", C.c_uint32),
                ("dCount", C.c_void_p)]


def trace_mode(name: str) -> int:
    """'flat' | 'octree' -> SAILOR_TRACE_*; anything else raises"""
    if name not in TRACE_MODES:
        raise ValueError(f"unknown trace mode {name!r}: expected one of {sorted(TRACE_MODES)}")
    return TRACE_MODES[name]


class EyeAdaptationConstants(C.Structure):  # include/sailor_hip.h SailorEyeAdaptationConstants (EyeAdaptationNode.cpp:154-170)
    _fields_ = [("minLog2Luminance", C.c_float), ("invLog2LuminanceRange", C.c_float), ("log2LuminanceRange", C.c_float),
                ("numPixels", C.c_float), ("timeCoeff", C.c_float)]


def tonemap_flags(defines: str) -> int:
    """'UNCHARTED2 LUMINANCE' (the node's toneMappingDefines string) -> SAILOR_TONEMAP_* bits; an unknown define raises"""
    flags = 0
    for name in defines.split():
        if name not in TONEMAP_DEFINES:
            raise ValueError(f"unknown tone-mapping define {name!r}: expected some of {sorted(TONEMAP_DEFINES)}")
        flags |= TONEMAP_DEFINES[name]
    return flags


class HbaoParams(C.Structure):  # include/sailor_hip.h SailorHbaoParams (HBAO.shader:50-57); defaults = DefaultRenderer.renderer:226-230
    _fields_ = [("occlusionRadius", C.c_float), ("occlusionPower", C.c_float), ("occlusionAttenuation", C.c_float), ("occlusionBias", C.c_float),
                ("noiseScale", C.c_float)]


class HbaoBlurParams(C.Structure):  # include/sailor_hip.h SailorHbaoBlurParams (HBAO_Blur.shader:54-59); DefaultRenderer.renderer:243-245
    _fields_ = [("sharpness", C.c_float), ("distanceScale", C.c_float), ("radius", C.c_float)]


HBAO_SHIPPED = dict(occlusionRadius=700.0, occlusionPower=1.5, occlusionAttenuation=0.1, occlusionBias=0.05, noiseScale=25.0)
HBAO_BLUR_SHIPPED = dict(sharpness=0.5, distanceScale=2.0, radius=5.0)


class MotionBlurParams(C.Structure):  # include/sailor_hip.h SailorMotionBlurParams (MotionBlur.shader:50-55); defaults = DefaultRenderer.renderer:328-330
    _fields_ = [("intensity", C.c_float), ("samples", C.c_float), ("maxSpeed", C.c_float)]


MOTION_BLUR_SHIPPED = dict(intensity=1.0, samples=10.0, maxSpeed=50.0)
DEBUG_VIEW_SCENE, DEBUG_VIEW_AO, DEBUG_VIEW_LIGHT_TILES, DEBUG_VIEW_CASCADES = 0, 1, 2, 3  # SAILOR_DEBUG_VIEW_*: Debug.shader's define sets
DEBUG_VIEW_MODES = {"": DEBUG_VIEW_SCENE, "AO": DEBUG_VIEW_AO, "LIGHT_TILES": DEBUG_VIEW_LIGHT_TILES, "CASCADES": DEBUG_VIEW_CASCADES}
SHADOW_CASCADE_LEVELS = (0.05, 0.1, 0.333333, 0.5)  # SAILOR_SHADOW_CASCADE_LEVELS (Constants.glsl)


class BlurParams(C.Structure):  # include/sailor_hip.h SailorBlurParams (Blur.shader:54-59): three vec4s
    _fields_ = [("blurRadius", C.c_float * 4), ("blurCenter", C.c_float * 4), ("blurSampleCount", C.c_float * 4)]


class ChromaticAberrationParams(C.Structure):  # include/sailor_hip.h SailorChromaticAberrationParams (ChromaticAberation.shader:52-55)
    _fields_ = [("offset", C.c_float * 4)]


BLUR_HORIZONTAL, BLUR_VERTICAL, BLUR_RADIAL = 1, 2, 4  # SAILOR_BLUR_*: Blur.shader's defines outside EVSM
BLUR_DEFINES = {"HORIZONTAL": BLUR_HORIZONTAL, "VERTICAL": BLUR_VERTICAL, "RADIAL": BLUR_RADIAL}
BLUR_GAUSS_SHIPPED = dict(blurRadius=(4.0, 2.0, 0.0, 0.0))  # DefaultRenderer.renderer:178 (a commented entry)
BLUR_RADIAL_SHIPPED = dict(blurRadius=(20.0, 0.0, 0.0, 0.0), blurSampleCount=(10.0, 0.0, 0.0, 0.0), blurCenter=(0.5, 0.5, 0.0, 0.0))  # :164-166
CHROMATIC_ABERRATION_SHIPPED = dict(offset=(0.00225, 0.00345, 0.00455, 0.0))  # :362


def blur_flags(defines: str) -> int:
    """'HORIZONTAL' | 'RADIAL VERTICAL' | '' (a PostProcess entry's `defines` string) -> SAILOR_BLUR_* bits; EVSM without RADIAL has its own entry point
    (sailor_hip_evsm_blur_pass) and raises here, like an unknown define; with RADIAL the shader never reaches its EVSM branch"""
    names = defines.split()
    flags = 0
    for name in names:
        if name == "EVSM" and "RADIAL" in names:
            continue
        if name not in BLUR_DEFINES:
            raise ValueError(f"no entry point for Blur.shader under {defines!r}: expected some of {sorted(BLUR_DEFINES)}")
        flags |= BLUR_DEFINES[name]
    return flags


class SkyParams(C.Structure):  # include/sailor_hip.h SailorSkyParams (Sky.shader:116-136 == SkyNode.h:48-67)
    _fields_ = [("lightDirection", C.c_float * 4), ("cloudsAttenuation1", C.c_float), ("cloudsAttenuation2", C.c_float), ("cloudsDensity", C.c_float),
                ("cloudsCoverage", C.c_float), ("phaseInfluence1", C.c_float), ("phaseInfluence2", C.c_float), ("eccentrisy1", C.c_float),
                ("eccentrisy2", C.c_float), ("fog", C.c_float), ("sunIntensity", C.c_float), ("ambient", C.c_float), ("scatteringSteps", C.c_int32),
                ("scatteringDensity", C.c_float), ("scatteringIntensity", C.c_float), ("scatteringPhase", C.c_float), ("sunShaftsIntensity", C.c_float),
                ("sunShaftsDistance", C.c_int32)]


SKY_RESOLUTION, SKY_SUN_RESOLUTION, SKY_ENV_CUBEMAP_SIZE, SKY_ENV_CUBEMAP_LEVELS = 256, 32, 256, 8  # SkyNode.h:13-15, SkyNode.cpp:755
SKY_STAR_TABLE_ROWS = 391  # sailor_host_sky_star_color_table: s_rgbTemperatures with the entry index 390 addresses


class BloomParams(C.Structure):  # include/sailor_hip.h SailorBloomParams; defaults = DefaultRenderer.renderer:298-302
    _fields_ = [("threshold", C.c_float), ("knee", C.c_float), ("bloomIntensity", C.c_float), ("dirtIntensity", C.c_float)]


BLOOM_SHIPPED = dict(threshold=3.0, knee=0.2, bloomIntensity=1.3, dirtIntensity=5.0)
BLOOM_SHIPPED_LEVELS = 8  # DefaultRenderer.renderer:24-31: Main, bGenerateMips, maxMipLevel 8


class HiZDesc(C.Structure):
    _fields_ = [("pyramid", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32)]


class IblDesc(C.Structure):  # include/sailor_hip.h SailorIblDesc (Standard.shader bindings 3, 4, 5, 9)
    _fields_ = [("irradiance", C.c_void_p), ("irrSize", C.c_int32), ("env", C.c_void_p), ("envSize", C.c_int32), ("envLevels", C.c_int32),
                ("brdfLut", C.c_void_p), ("lutW", C.c_int32), ("lutH", C.c_int32), ("ao", C.c_void_p)]


class VertexP3N3T3B3UV2C4(C.Structure):  # RHI/Types.h:720-727, interleaved
    _fields_ = [("texcoord", C.c_float * 2), ("position", C.c_float * 3), ("normal", C.c_float * 3), ("tangent", C.c_float * 3),
                ("bitangent", C.c_float * 3), ("color", C.c_float * 4)]


class MaterialData(C.Structure):  # Standard.shader:164-178, std430
    _fields_ = [("albedo", C.c_float * 4), ("ambient", C.c_float * 4), ("emission", C.c_float * 4), ("metallic", C.c_float), ("roughness", C.c_float),
                ("ao", C.c_float), ("albedoSampler", C.c_uint32), ("metalnessSampler", C.c_uint32), ("normalSampler", C.c_uint32),
                ("roughnessSampler", C.c_uint32), ("_pad", C.c_uint32)]


class GltfMaterialData(C.Structure):  # Standard_glTF.shader:42-58, std430
    _fields_ = [("baseColorFactor", C.c_float * 4), ("emissiveFactor", C.c_float * 4), ("metallicFactor", C.c_float), ("roughnessFactor", C.c_float),
                ("occlusionStrength", C.c_float), ("normalScale", C.c_float), ("alphaCutoff", C.c_float), ("baseColorSampler", C.c_uint32),
                ("normalSampler", C.c_uint32), ("ormSampler", C.c_uint32), ("occlusionSampler", C.c_uint32), ("emissiveSampler", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class TextureDesc(C.Structure):  # include/sailor_hip.h SailorTextureDesc: one entry of Standard.shader:124 textureSamplers[]
    _fields_ = [("texels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_uint32), ("levels", C.c_uint32)]


class SurfaceDraw(C.Structure):  # include/sailor_hip.h SailorSurfaceDraw: one DrawIndexed of RenderSceneNode.cpp
    _fields_ = [("dVertices", C.c_void_p), ("dIndices", C.c_void_p), ("dInstanceIds", C.c_void_p), ("numTriangles", C.c_uint32), ("numDrawn", C.c_uint32),
                ("primBase", C.c_uint32), ("flags", C.c_uint32), ("firstInstance", C.c_uint32), ("_pad", C.c_uint32)]


class DebugLinesDraw(C.Structure):  # include/sailor_hip.h SailorDebugLinesDraw: the one DrawIndexed of DebugContext::DrawDebugMesh
    _fields_ = [("dVertices", C.c_void_p), ("dIndices", C.c_void_p), ("numSegments", C.c_uint32), ("primBase", C.c_uint32)]


class UiCommand(C.Structure):  # include/sailor_hip.h SailorUiCommand: one DrawIndexed of ImGui_RenderDrawData under its scissor
    _fields_ = [("firstIndex", C.c_uint32), ("indexCount", C.c_uint32), ("vertexOffset", C.c_int32), ("scissor", C.c_int32 * 4)]


class UiDrawCmd(C.Structure):  # include/sailor_hip.h SailorUiDrawCmd: what an ImDrawCmd holds
    _fields_ = [("clipRect", C.c_float * 4), ("elemCount", C.c_uint32), ("idxOffset", C.c_uint32), ("vtxOffset", C.c_uint32), ("callback", C.c_uint32)]


class UiDrawList(C.Structure):  # include/sailor_hip.h SailorUiDrawList: an ImDrawList's buffer sizes and its run of commands
    _fields_ = [("vtxCount", C.c_uint32), ("idxCount", C.c_uint32), ("firstCmd", C.c_uint32), ("cmdCount", C.c_uint32)]


VERTEX_P3C4_DTYPE = [("position", "<f4", 3), ("color", "<f4", 4)]  # SailorVertexP3C4, 28 bytes
VERTEX_P2UV2C1_DTYPE = [("position", "<f4", 2), ("uv", "<f4", 2), ("color", "<u4")]  # SailorVertexP2UV2C1, 20 bytes, r in the low byte
UI_COMMAND_DTYPE = [("firstIndex", "<u4"), ("indexCount", "<u4"), ("vertexOffset", "<i4"), ("scissor", "<i4", 4)]  # SailorUiCommand, 28 bytes
UI_MAX_COMMANDS = 16384  # SAILOR_UI_MAX_COMMANDS
UI_CALLBACK_NONE, UI_CALLBACK_RESET, UI_CALLBACK_USER = 0, 1, 2  # SAILOR_UI_CALLBACK_*
TEXTURE_SRGB = 1        # SAILOR_TEXTURE_SRGB
SURFACE_CULL_BACK = 1   # SAILOR_SURFACE_CULL_BACK
SURFACE_ALPHA_CUTOUT = 2  # SAILOR_SURFACE_ALPHA_CUTOUT (sailor_hip_surface_draw_masked only)
SURFACE_GLTF = 4        # SAILOR_SURFACE_GLTF (sailor_hip_surface_draw_gltf only)
SURFACE_BLEND_SHIFT, SURFACE_BLEND_MASK = 3, 3   # SAILOR_SURFACE_BLEND_SHIFT / _MASK (sailor_hip_surface_peel_draw / _peel_draw_gltf only)
SURFACE_BLEND_NONE, SURFACE_BLEND_ADDITIVE, SURFACE_BLEND_ALPHA, SURFACE_BLEND_MULTIPLY = 0, 1, 2, 3   # EBlendMode; MULTIPLY is refused
SURFACE_BLEND_MODES = {"none": SURFACE_BLEND_NONE, "additive": SURFACE_BLEND_ADDITIVE, "alpha": SURFACE_BLEND_ALPHA, "multiply": SURFACE_BLEND_MULTIPLY}
# the same records as NumPy dtypes (what the tests and upload helpers build)
VERTEX_DTYPE = [("texcoord", "<f4", 2), ("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("bitangent", "<f4", 3), ("color", "<f4", 4)]
MATERIAL_DTYPE = [("albedo", "<f4", 4), ("ambient", "<f4", 4), ("emission", "<f4", 4), ("metallic", "<f4"), ("roughness", "<f4"), ("ao", "<f4"),
                  ("albedoSampler", "<u4"), ("metalnessSampler", "<u4"), ("normalSampler", "<u4"), ("roughnessSampler", "<u4"), ("_pad", "<u4")]
# SailorGltfMaterialData (Standard_glTF.shader:42-58, std430): the same 80-byte slot of the one material table, read by a draw that carries SURFACE_GLTF
GLTF_MATERIAL_DTYPE = [("baseColorFactor", "<f4", 4), ("emissiveFactor", "<f4", 4), ("metallicFactor", "<f4"), ("roughnessFactor", "<f4"),
                       ("occlusionStrength", "<f4"), ("normalScale", "<f4"), ("alphaCutoff", "<f4"), ("baseColorSampler", "<u4"), ("normalSampler", "<u4"),
                       ("ormSampler", "<u4"), ("occlusionSampler", "<u4"), ("emissiveSampler", "<u4"), ("_pad", "<u4", 2)]

class ParticleData(C.Structure):  # include/sailor_hip.h SailorParticleData (ParticlesNode.h:44-51)
    _fields_ = [("enabled", C.c_float), ("size1", C.c_float), ("size2", C.c_float), ("_nouse", C.c_float), ("xyz1", C.c_float * 3), ("_w1", C.c_float),
                ("rgba1", C.c_float * 4), ("xyz2", C.c_float * 3), ("_w2", C.c_float), ("rgba2", C.c_float * 4)]


class ParticleInstance(C.Structure):  # include/sailor_hip.h SailorParticleInstance (ParticlesNode.h:62-71, std430)
    _fields_ = [("model", C.c_float * 16), ("color", C.c_float * 4), ("colorOld", C.c_float * 4), ("materialInstance", C.c_uint32), ("isCulled", C.c_uint32),
                ("_pad", C.c_uint32 * 2)]


class ParticlesConstants(C.Structure):  # include/sailor_hip.h SailorParticlesConstants (ParticlesNode.h:53-60)
    _fields_ = [("numInstances", C.c_uint32), ("numFrames", C.c_uint32), ("fps", C.c_uint32), ("traceFrames", C.c_uint32), ("traceDecay", C.c_float)]


class ParticlesDraw(C.Structure):  # include/sailor_hip.h SailorParticlesDraw: the particle mesh
    _fields_ = [("dVertices", C.c_void_p), ("dIndices", C.c_void_p), ("numTriangles", C.c_uint32), ("_pad", C.c_uint32)]


PARTICLE_DATA_DTYPE = [("enabled", "<f4"), ("size1", "<f4"), ("size2", "<f4"), ("_nouse", "<f4"), ("xyz1", "<f4", 3), ("_w1", "<f4"), ("rgba1", "<f4", 4),
                       ("xyz2", "<f4", 3), ("_w2", "<f4"), ("rgba2", "<f4", 4)]  # SailorParticleData, 80 bytes
PARTICLE_INSTANCE_DTYPE = [("model", "<f4", 16), ("color", "<f4", 4), ("colorOld", "<f4", 4), ("materialInstance", "<u4"), ("isCulled", "<u4"),
                           ("_pad", "<u4", 2)]  # SailorParticleInstance, 112 bytes
assert C.sizeof(ParticleData) == 80 and C.sizeof(ParticleInstance) == 112 and C.sizeof(ParticlesConstants) == 20 and C.sizeof(ParticlesDraw) == 24

assert C.sizeof(VertexP3N3T3B3UV2C4) == 72 and C.sizeof(MaterialData) == 80 and C.sizeof(GltfMaterialData) == 80
assert C.sizeof(TextureDesc) == 24 and TextureDesc.levels.offset == 20 and C.sizeof(SurfaceDraw) == 48
assert C.sizeof(UboFrameData) == 232 and C.sizeof(LightCullPushConstants) == 88 and C.sizeof(LightShaderData) == 112

_P = C.c_void_p
# name -> (restype, argtypes); one entry per symbol declared in include/sailor_hip.h
SIGNATURES = {
    "sailor_hip_version": (C.c_int, []),
    "sailor_hip_status_string": (C.c_char_p, [C.c_int]),
    "sailor_hip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "sailor_hip_context_create": (C.c_int, [C.c_int, _P, C.c_uint32, C.POINTER(_P)]),
    "sailor_hip_context_destroy": (C.c_int, [_P]),
    "sailor_hip_context_synchronize": (C.c_int, [_P]),
    "sailor_hip_context_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "sailor_hip_context_last_error": (C.c_char_p, [_P]),
    "sailor_hip_buffer_create": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "sailor_hip_buffer_free": (C.c_int, [_P, _P]),
    "sailor_hip_buffer_upload": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "sailor_hip_buffer_download": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_size_t]),
    "sailor_hip_buffer_fill_u32": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_size_t]),
    "sailor_hip_num_tiles": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sailor_hip_band_whole_frame": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_band_from_tile_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_band_for_rank": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_band_is_valid": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_light_cull_workspace_size": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_light_cull": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(LightCullPushConstants), _P, _P, _P, _P, C.c_size_t,
                                        _P, C.c_size_t, C.POINTER(Band), C.c_uint32]),
    "sailor_hip_linearize_depth": (C.c_int, [_P, C.POINTER(UboFrameData), _P, _P, C.c_int32, C.c_int32]),
    "sailor_hip_light_cull_diagnostics": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.POINTER(C.c_uint64)]),
    "sailor_hip_light_grid_rebase": (C.c_int, [_P, _P, C.c_int32, C.c_uint32]),
    "sailor_hip_shade": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_size_t, _P, C.c_int32, _P, _P, C.POINTER(CsmDesc), _P, C.POINTER(Band)]),
    "sailor_hip_shade_ex": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_size_t, _P, C.c_int32, _P, _P, C.POINTER(CsmDesc), C.POINTER(IblDesc), _P,
                                      C.POINTER(Band), _P]),
    "sailor_hip_prepared_lights_size": (C.c_size_t, [C.c_int32]),
    "sailor_hip_prepare_lights": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_size_t]),
    "sailor_hip_prepared_lights_views": (C.c_int, [C.c_int32, _P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "sailor_hip_light_cull_prepared": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(LightCullPushConstants), _P, _P, _P, _P, C.c_size_t,
                                                 _P, C.c_size_t, C.POINTER(Band), C.c_uint32, _P, C.c_int32]),
    "sailor_hip_shade_prepared": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_size_t, _P, C.c_int32, _P, _P, C.POINTER(CsmDesc), C.POINTER(IblDesc), _P,
                                            C.POINTER(Band), _P, _P, C.c_int32]),
    "sailor_hip_light_cull_tile_order": (_P, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band), _P]),
    "sailor_hip_light_cull_tile_lists": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.POINTER(_P), C.POINTER(_P)]),
    "sailor_hip_light_cull_pack": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band), _P, _P, _P, C.c_size_t]),
    "sailor_hip_shade_tile_lists": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_size_t, _P, C.c_int32, _P, _P, C.POINTER(CsmDesc), C.POINTER(IblDesc), _P,
                                              C.POINTER(Band), _P, _P, C.c_int32]),
    "sailor_hip_context_wait_for": (C.c_int, [_P, _P]),
    "sailor_hip_context_time_launches": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "sailor_hip_context_timed_launch_ms": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_float)]),
    "sailor_hip_copy_probe": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "sailor_hip_marker": (C.c_int, [_P]),
    "sailor_hip_context_launch_log": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p), C.c_int32]),
    "sailor_hip_light_cull_band_selection": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.POINTER(_P), C.POINTER(_P)]),
    "sailor_hip_evsm_blur": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_evsm_blur_pass": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_compute_brdf_lut": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "sailor_hip_self_check_exact_math": (C.c_int, [_P, _P, C.POINTER(C.c_uint64)]),
    "sailor_hip_compute_irradiance_map": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "sailor_hip_prefilter_env_map": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "sailor_hip_equirect_to_cube": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_generate_mipmaps_cube": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "sailor_hip_prefilter_env_level": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float]),
    "sailor_hip_buffer_copy": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.c_size_t]),
    "sailor_hip_ecs_sweep": (C.c_int, [_P, C.c_uint32, _P, _P, C.POINTER(C.c_uint32), C.c_uint32, _P, C.POINTER(C.c_float), _P, _P, _P]),
    "sailor_hip_ecs_sweep_range": (C.c_int, [_P, C.c_uint32, _P, _P, C.POINTER(C.c_uint32), C.c_uint32, _P, C.POINTER(C.c_float), _P, _P, _P, C.c_uint32, C.c_uint32]),
    "sailor_hip_ecs_sweep_traced": (C.c_int, [_P, C.c_uint32, _P, _P, C.POINTER(C.c_uint32), C.c_uint32, _P, C.POINTER(C.c_float), _P, _P, _P, C.c_uint32,
                                              C.c_uint32, C.POINTER(SceneTrace)]),
    "sailor_hip_ecs_range_for_rank": (C.c_int, [C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "sailor_hip_exchange_adapt": (C.c_int, [_P, _P, _P, _P]),
    "sailor_hip_exchange_set_slot_words": (C.c_int, [_P, C.c_size_t]),
    "sailor_hip_exchange_visibility": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_uint32, _P, C.c_size_t]),
    "sailor_hip_mesh_frustum_cull": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_uint32, C.c_uint32]),
    "sailor_hip_raster_coarse_words": (C.c_size_t, [C.c_int32, C.c_int32]),
    "sailor_hip_raster_depth": (C.c_int, [_P, C.POINTER(C.c_float), _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_int32, C.c_int32, _P, C.c_uint32, _P]),
    "sailor_hip_raster_depth_camera": (C.c_int, [_P, C.POINTER(UboFrameData), _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_int32, C.c_int32, _P, C.c_uint32, _P]),
    "sailor_hip_shadow_resolve": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    "sailor_hip_csm_caster_masks": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_float), C.c_uint32, _P]),
    "sailor_hip_csm_caster_masks_traced": (C.c_int, [_P, C.c_uint32, _P, C.POINTER(C.c_float), C.c_uint32, _P, C.POINTER(SceneTrace)]),
    "sailor_hip_shadow_gather_workspace_bytes": (C.c_size_t, [C.POINTER(ShadowGatherJob), C.c_uint32]),
    "sailor_hip_shadow_gather_instances_batched": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(ShadowGatherJob), C.c_uint32, _P, C.c_size_t]),
    "sailor_hip_shadow_gather_instances": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, C.c_size_t]),
    "sailor_hip_buffer_fill_pattern": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint32, C.c_size_t]),
    "sailor_hip_shadow_extract_positions": (C.c_int, [_P, _P, C.c_uint32, _P]),
    "sailor_hip_hiz_downscale": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_hiz_build": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_mesh_cull_flags": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_uint32, C.c_uint32, C.POINTER(HiZDesc)]),
    "sailor_hip_mesh_cull_compact_ex": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_size_t, C.POINTER(HiZDesc)]),
    "sailor_hip_mesh_cull_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "sailor_hip_mesh_cull_compact": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, C.c_size_t]),
    "sailor_hip_eye_adaptation_state_size": (C.c_size_t, []),
    "sailor_hip_eye_adaptation_reset": (C.c_int, [_P, _P, C.c_float]),
    "sailor_hip_eye_adaptation_state_views": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "sailor_hip_luminance_histogram": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(Band), C.POINTER(EyeAdaptationConstants), _P]),
    "sailor_hip_average_luminance": (C.c_int, [_P, C.POINTER(EyeAdaptationConstants), _P]),
    "sailor_hip_tonemap": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(Band), C.c_uint32, C.POINTER(C.c_float), C.c_float, _P]),
    "sailor_hip_eye_adaptation": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(EyeAdaptationConstants), C.c_uint32, C.POINTER(C.c_float),
                                            C.c_float, _P]),
    "sailor_host_eye_adaptation_constants": (C.c_int, [C.c_int32, C.c_int32, C.c_float, C.POINTER(EyeAdaptationConstants)]),
    "sailor_hip_blit_nearest": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_hbao": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(HbaoParams), _P, C.c_int32,
                                  C.c_int32]),
    "sailor_hip_hbao_blur_pass": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(HbaoBlurParams), _P, C.c_int32, C.c_int32,
                                            C.c_int32]),
    "sailor_hip_hbao_chain": (C.c_int, [_P, C.POINTER(UboFrameData), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32,
                                        C.POINTER(HbaoParams), _P, C.c_int32, C.c_int32, C.POINTER(HbaoBlurParams), _P, C.c_int32, C.c_int32, _P, C.c_int32,
                                        C.c_int32]),
    "sailor_hip_motion_blur": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(UboFrameData), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32,
                                         C.POINTER(MotionBlurParams), _P, C.c_int32, C.c_int32]),
    "sailor_hip_debug_view": (C.c_int, [_P, C.POINTER(UboFrameData), C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32,
                                        C.c_int32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_blur": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(BlurParams), C.c_uint32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_chromatic_aberration": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(ChromaticAberrationParams), _P, C.c_int32, C.c_int32]),
    "sailor_hip_blit_linear": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_sky_fill": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32]),
    "sailor_hip_sky_env_face": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32]),
    "sailor_hip_sky_sun": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_sky_compose": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P,
                                         C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_sky_env_cubemap": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32]),
    "sailor_hip_sky_clouds": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32,
                                        _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_sky_sun_clouds": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32]),
    "sailor_hip_sky_blit_clouds": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_sky_sun_shafts": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SkyParams), _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32,
                                            C.POINTER(Band)]),
    "sailor_hip_sky_stars_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "sailor_hip_sky_stars_bind_workspace": (C.c_int, [_P, _P, C.c_size_t]),
    "sailor_hip_sky_stars": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(C.c_float), _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, C.c_int32,
                                       C.c_int32, C.POINTER(Band)]),
    "sailor_host_sky_sun_color": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_sky_star_color_table": (C.c_int, [C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_float)]),
    "sailor_host_sky_star_mesh": (C.c_int, [_P, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32,
                                            C.POINTER(C.c_uint32)]),
    "sailor_host_sky_stars_model": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_sky_params_default": (C.c_int, [C.POINTER(SkyParams)]),
    "sailor_host_sky_face_matrices": (C.c_int, [C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_hip_mip_chain_texels": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_bloom_downscale": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32]),
    "sailor_hip_bloom_upscale": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, C.c_int32, C.c_int32]),
    "sailor_hip_bloom": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(BloomParams), _P, C.c_int32, C.c_int32]),
    "sailor_host_bloom_push_constants": (C.c_int, [C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "sailor_hip_allgather_u32": (C.c_int, [_P, _P, _P, _P, C.c_size_t]),
    "sailor_hip_exchange_workspace_size": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_exchange_light_lists": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t]),
    "sailor_hip_stitch_light_lists": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_size_t]),
    "sailor_hip_exchange_workspace_size_rows": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, _P]),
    "sailor_hip_exchange_light_lists_rows": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t]),
    "sailor_hip_stitch_light_lists_rows": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_size_t]),
    "sailor_host_perspective_rh": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "sailor_host_mat4_inverse": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_mat4_mul": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_transform_matrix": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_fill_frame_data": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32,
                                              C.c_float, C.c_float, C.POINTER(UboFrameData)]),
    "sailor_host_extract_frustum_planes": (C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float,
                                                     C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_extract_frustum_planes_matrix": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_csm_matrices": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float,
                                           C.POINTER(C.c_float)]),
    "sailor_host_overlaps_sphere": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_contains_sphere": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sailor_host_lights_in_frustum": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint32),
                                                _P, _P, C.POINTER(C.c_uint32), _P, _P, C.POINTER(C.c_uint32)]),
    "sailor_host_csm_snapshots_create": (_P, []),
    "sailor_host_csm_snapshots_clone": (_P, [_P]),
    "sailor_host_csm_snapshots_destroy": (None, [_P]),
    "sailor_host_csm_snapshots_count": (C.c_uint32, [_P]),
    "sailor_host_csm_snapshot_get": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), _P, _P, C.POINTER(C.c_int32), C.POINTER(CsmView)]),
    "sailor_host_csm_plan_passes": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, C.POINTER(CsmView), _P, _P]),
    "sailor_host_pack_light": (C.c_int, [C.c_uint32, C.c_uint32] + [C.POINTER(C.c_float)] * 6 + [C.POINTER(LightShaderData)]),
    "sailor_hip_surface_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.POINTER(Band), C.c_uint32]),
    "sailor_hip_surface_begin": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_surface_draw": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_surface_resolve": (C.c_int, [_P, C.POINTER(UboFrameData), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t,
                                             _P, C.c_size_t, _P, _P]),
    "sailor_hip_surface_composite": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_surface_draw_masked": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                                 C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_surface_store_depth": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_surface_draw_gltf": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                               C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_surface_resolve_gltf": (C.c_int, [_P, C.POINTER(UboFrameData), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t,
                                                  _P, C.c_size_t, _P, _P, _P, _P, _P]),
    "sailor_hip_surface_composite_gltf": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_surface_draw_indirect": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32,
                                                   C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_texture_mip_levels": (C.c_uint32, [C.c_int32, C.c_int32]),
    "sailor_host_srgb_encode_table": (C.c_int, [C.POINTER(C.c_float)]),
    "sailor_hip_texture_generate_mips": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32]),
    "sailor_hip_surface_resolve_lod": (C.c_int, [_P, C.POINTER(UboFrameData), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t,
                                                 _P, C.c_size_t, _P, _P, _P, _P, _P]),
    "sailor_hip_surface_draw_lod": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                              C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_surface_draw_indirect_lod": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32,
                                                       C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_surface_peel_begin": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, C.c_int32]),
    "sailor_hip_surface_peel_draw": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                               C.POINTER(Band), _P, C.c_size_t, _P, _P]),
    "sailor_hip_surface_peel_draw_gltf": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32,
                                                    C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, _P]),
    "sailor_hip_surface_peel_commit": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, _P]),
    "sailor_hip_surface_blend": (C.c_int, [_P, _P, _P, _P, _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_surface_bucket_bytes": (C.c_size_t, [C.c_int32, C.POINTER(Band), C.c_uint32]),
    "sailor_hip_surface_bucket_begin": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, C.c_size_t, C.c_uint32]),
    "sailor_hip_surface_bucket_draw": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                                 C.POINTER(Band), _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32]),
    "sailor_hip_surface_bucket_draw_gltf": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32,
                                                      C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, _P, C.c_size_t, C.c_uint32]),
    "sailor_hip_surface_bucket_layer": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, C.c_size_t, C.c_uint32, C.c_uint32, _P]),
    "sailor_host_msaa_sample_positions": (C.c_int, [C.c_uint32, _P]),
    "sailor_hip_surface_msaa_bytes": (C.c_size_t, [C.c_int32, C.POINTER(Band), C.c_uint32]),
    "sailor_hip_surface_msaa_begin": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, C.c_size_t, C.c_uint32, _P]),
    "sailor_hip_surface_msaa_draw": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                               C.POINTER(Band), _P, C.c_size_t, _P, C.c_size_t, C.c_uint32]),
    "sailor_hip_surface_msaa_draw_gltf": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(SurfaceDraw), _P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_int32,
                                                    C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, C.c_size_t, C.c_uint32]),
    "sailor_hip_surface_msaa_layer": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P,
                                                _P]),
    "sailor_hip_surface_msaa_accumulate": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_surface_msaa_store_depth": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, _P, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_hip_surface_keys_offset": (C.c_size_t, []),
    "sailor_host_srgb_table": (C.c_int, [C.POINTER(C.c_float)]),
    "sailor_hip_surface_draw_prims": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "sailor_hip_debug_lines_draw": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(DebugLinesDraw), C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t]),
    "sailor_hip_debug_lines_resolve": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(DebugLinesDraw), C.c_int32, C.c_int32, C.POINTER(Band), _P, C.c_size_t, _P, _P]),
    "sailor_hip_debug_lines_prims": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint64)]),
    "sailor_hip_ui_workspace_bytes": (C.c_int, [C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "sailor_hip_ui_draw": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(TextureDesc), _P, C.c_size_t, _P, C.c_int32, C.c_int32, C.POINTER(Band)]),
    "sailor_host_ui_flatten": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(UiDrawList), C.c_uint32, C.POINTER(UiDrawCmd),
                                         C.c_uint32, C.POINTER(C.c_float), C.POINTER(UiCommand), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32)]),
    "sailor_hip_particles_update": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(ParticlesConstants), _P, C.c_uint32, _P]),
    "sailor_hip_particles_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sailor_hip_particles_shadow": (C.c_int, [_P, C.POINTER(ParticlesDraw), _P, C.c_uint32, _P, _P, C.c_int32, C.c_int32, _P, C.c_size_t]),
    "sailor_hip_particles_draw": (C.c_int, [_P, C.POINTER(UboFrameData), C.POINTER(ParticlesDraw), _P, C.c_uint32, _P, _P, _P, C.c_int32, C.c_int32, _P, _P,
                                            C.c_int32, C.c_int32, _P, C.c_size_t]),
}

_lib = None


def load() -> C.CDLL:
    """Load libsailor_hip.so (built in-tree by __graft_entry__.build() / `make -C sailor_amd/csrc`)."""
    global _lib
    if _lib is None:
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so).  Streams and device pointers are handed across this
        # boundary, so both sides must live in ONE runtime instance: import torch first and let the loader resolve our
        # libamdhip64 dependency to the copy that is already mapped.
        import torch  # noqa: F401
        path = Path(os.environ.get("SAILOR_HIP_LIB", LIB_PATH))
        if not path.exists():
            raise SailorHipError(-2, "load", f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                             "or `make -C sailor_amd/csrc` (there is no CPU fallback)")
        lib = C.CDLL(str(path))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here == the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def status_string(status: int) -> str:
    try:
        return load().sailor_hip_status_string(status).decode()
    except Exception:  # library itself unavailable
        return "?"


def check(status: int, where: str, ctx=None) -> None:
    if status != 0:
        detail = ""
        if ctx is not None:
            detail = load().sailor_hip_context_last_error(ctx).decode()
        raise SailorHipError(status, where, detail)


def call(name: str, *args) -> None:
    """the checked call of the entry `name`, one that takes no context (HipContext.call is the one for those that do): a status other than 0 raises under
    the entry's name"""
    check(getattr(load(), name)(*args), name)
