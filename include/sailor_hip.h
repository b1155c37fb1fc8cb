/*
 * sailor_hip.h -- C-ABI of the MI355X-native Forward+ lighting path for the Sailor engine.
 *
 * This is the drop-in boundary: the only thing `Runtime/GraphicsDriver/HIP` (the new RHI backend that sits
 * beside the reference's `Runtime/GraphicsDriver/Vulkan`) calls.  Style follows the reference's own exported
 * C surface, Lib/DllMain.cpp:9-160: `extern "C"`, cdecl, POD arguments, integer status returns.
 *
 * Conventions
 *   - every entry point returns `int`: 0 = SAILOR_HIP_OK, negative = error class (table below); nothing throws;
 *   - entry points RECORD work on the context's stream and return without synchronising (mirrors the reference's
 *     record-then-submit model: RHI/GraphicsDriver.h:310-314 Dispatch, :149 SubmitCommandList); only
 *     sailor_hip_context_synchronize / sailor_hip_buffer_download wait;
 *   - no allocation on the caller's behalf except through sailor_hip_buffer_create; kernels take raw device
 *     pointers, so memory owned by another allocator (a torch tensor, an engine heap) is accepted as is;
 *   - thread-compatible per context (one stream per context; the reference calls from the one Render thread,
 *     RHI/Renderer.cpp:264-303);
 *   - matrices are column-major float[16] exactly as glm::mat4 lies in memory.
 *
 * There is NO CPU fallback behind this header: if the HIP runtime or a gfx950 device is missing every
 * device entry point fails with SAILOR_HIP_ERR_NO_DEVICE.
 */
#ifndef SAILOR_HIP_H
#define SAILOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(SAILOR_HIP_BUILD)
#define SAILOR_HIP_API __attribute__((visibility("default")))
#else
#define SAILOR_HIP_API
#endif

/* ---- status codes ------------------------------------------------------------------------------------ */
#define SAILOR_HIP_OK 0
#define SAILOR_HIP_ERR_INVALID_ARGUMENT (-1)
#define SAILOR_HIP_ERR_NO_DEVICE (-2)       /* HIP runtime present but no usable device / wrong ordinal     */
#define SAILOR_HIP_ERR_OUT_OF_MEMORY (-3)
#define SAILOR_HIP_ERR_LAUNCH (-4)          /* kernel launch or stream operation failed                      */
#define SAILOR_HIP_ERR_WORKSPACE_TOO_SMALL (-5)
#define SAILOR_HIP_ERR_RCCL (-6)
#define SAILOR_HIP_ERR_UNSUPPORTED (-7)

/* ---- constants generated into Constants.glsl by AssetRegistry/Shader/ShaderCompiler.cpp:141-167 -------- */
#define SAILOR_LIGHTS_CULLING_TILE_SIZE 16     /* Constants.glsl:13 ; FrameGraph/LightCullingNode.h:16 */
#define SAILOR_LIGHTS_CANDIDATES_PER_TILE 196  /* Constants.glsl:14 */
#define SAILOR_LIGHTS_PER_TILE 128             /* Constants.glsl:15 ; FrameGraph/LightCullingNode.h:15 */
#define SAILOR_GPU_CULLING_GROUP_SIZE 256      /* Constants.glsl:18 ; RHI/Renderer.h:32 */
#define SAILOR_NUM_CSM_CASCADES 4              /* Constants.glsl:23 ; ECS/LightingECS.h:65 */
#define SAILOR_SHADOW_CASCADE_LEVELS { 0.05f, 0.1f, 0.333333f, 0.5f } /* Constants.glsl ShadowCascadeLevels (tests/golden/reference_constants.json), fractions of zFar */
#define SAILOR_LIGHTS_MAX_NUM 65535            /* ECS/LightingECS.h:54 (the reference's SSBO capacity) */

/* ---- POD mirrors of the reference's GPU-visible structs ------------------------------------------------ */

/* RHI/Types.h:751-761 UboFrameData, filled at FrameGraph/RHIFrameGraph.cpp:60-67.  232 bytes. */
typedef struct SailorUboFrameData {
    float view[16];
    float projection[16];
    float invProjection[16];
    float cameraPosition[4];
    int32_t viewportSize[2];
    float cameraZNearZFar[2];
    float currentTime;
    float deltaTime;
} SailorUboFrameData;

/* FrameGraph/LightCullingNode.h:25-31 PushConstants == ComputeLightCulling.shader:12-18.  88 bytes. */
typedef struct SailorLightCullPushConstants {
    float invViewProjection[16]; /* never read by the shader; kept for layout */
    int32_t viewportSize[2];
    int32_t numTiles[2];
    int32_t lightsNum;
    int32_t _pad;
} SailorLightCullPushConstants;

/* ECS/LightingECS.h:71-81 LightShaderData == Lighting.glsl:4-15 LightData.  std430, 112 bytes. */
typedef struct SailorLightShaderData {
    uint32_t type;       /* Engine/Types.h:31-37: 0 Directional, 1 Point, 2 Spot, 3 Area */
    uint32_t shadowType; /* RHI/SceneView.h:13-18: 0 None, 1 PCF, 2 EVSM */
    uint32_t _pad0[2];
    float worldPosition[3]; float _pad1;
    float direction[3];     float _pad2;
    float intensity[3];     float _pad3;
    float attenuation[3];   float _pad4;
    float cutOff[2];        float _pad5[2]; /* cosines, ECS/LightingECS.cpp:171 */
    float bounds[3];        float _pad6;
} SailorLightShaderData;

/* Lighting.glsl:17-22 LightsGrid */
typedef struct SailorLightsGrid {
    uint32_t offset;
    uint32_t num;
} SailorLightsGrid;

/* FrameGraph/RenderSceneNode.h:16-33 PerInstanceData == ComputeMeshCulling.shader:20-26.  96 bytes. */
typedef struct SailorPerInstanceData {
    float model[16];
    float sphereBounds[4];
    uint32_t materialInstance;
    uint32_t isCulled;
    uint32_t _pad[2];
} SailorPerInstanceData;

/* RHI/Types.h DrawIndexedIndirectData == VkDrawIndexedIndirectCommand == ComputeMeshCulling.shader:28-35.  20 bytes. */
typedef struct SailorDrawIndexedIndirectData {
    uint32_t indexCount;
    uint32_t instanceCount;
    uint32_t firstIndex;
    int32_t vertexOffset;
    uint32_t firstInstance;
} SailorDrawIndexedIndirectData;

/* Math/Transform.h: {vec4 m_position; quat m_rotation (memory x,y,z,w); vec4 m_scale}.  48 bytes. */
typedef struct SailorTransform {
    float position[4];
    float rotation[4];
    float scale[4];
} SailorTransform;

/* Math/Bounds.h:110-113 AABB {vec3 m_min; vec3 m_max}.  24 bytes. */
typedef struct SailorAABB {
    float min[3];
    float max[3];
} SailorAABB;

/* Shadow-map texel formats (ECS/LightingECS.h:57-58 + a plain fp32 form for tests) */
#define SAILOR_SHADOWMAP_R16_SFLOAT 0
#define SAILOR_SHADOWMAP_R32G32B32A32_SFLOAT 1
#define SAILOR_SHADOWMAP_R32_SFLOAT 2

/* The CSM inputs of Standard.shader: binding 6 `lightsMatrices` and binding 8 `shadowMaps[cascade]`
 * (Standard.shader:223-233).  Maps are linear row-major images in device memory, row 0 first.
 * (An R16F cascade of up to 8192 x 8192 texels has the sixteen PCF taps of a pixel read as one 6 x 6-texel window -- Lighting.glsl:168-197's
 * disk is +-2 texels --, a larger one tap by tap: the same bits either way; tests/test_shade_gpu.py runs both against the oracle.) */
typedef struct SailorCsmDesc {
    float lightsMatrices[SAILOR_NUM_CSM_CASCADES][16];
    const void* maps[SAILOR_NUM_CSM_CASCADES]; /* device pointers; NULL = no map bound => shadow factor 1 */
    int32_t width[SAILOR_NUM_CSM_CASCADES];
    int32_t height[SAILOR_NUM_CSM_CASCADES];
    int32_t format[SAILOR_NUM_CSM_CASCADES];
} SailorCsmDesc;

/* The image-based-lighting inputs of Standard.shader's AmbientLighting (:343-372): binding 3 `g_irradianceCubemap`, binding 4
 * `g_brdfSampler`, binding 5 `g_envCubemap`, binding 9 `g_aoSampler` (:219-221,234).  All device pointers, fp32 texels (the
 * reference keeps RGBA16F / RG16F images).  Canonical sampler (identical in the oracle): cube face and (s, t) by the Vulkan
 * major-axis table (ties z over y over x), bilinear inside the face with clamp-to-edge, linear between the two nearest mip
 * levels with lod clamped to [0, levels - 1]; 2-D: bilinear, clamp-to-edge. */
typedef struct SailorIblDesc {
    const float* irradiance; /* 6 faces (+X,-X,+Y,-Y,+Z,-Z) x irrSize^2 float4, face-major, row t = 0 first */
    int32_t irrSize;
    const float* env;        /* mip chain, level-major: level l = 6 faces x max(1, envSize >> l)^2 float4 */
    int32_t envSize;
    int32_t envLevels;       /* textureQueryLevels(g_envCubemap) (:361) */
    const float* brdfLut;    /* lutH x lutW float2 (DFG1, DFG2), u = cosLo, v = roughness (ComputeBrdfLut.shader) */
    int32_t lutW;
    int32_t lutH;
    const float* ao;         /* band rows x width floats: the g_aoSampler target at this pixel (:386); NULL = 1.0 */
} SailorIblDesc;

/*
 * A horizontal band of the frame: tile rows [tileRowBegin, tileRowEnd) of the light grid.  Tile row t covers
 * framebuffer rows H-1-16t-15 .. H-1-16t, so the band's pixels are framebuffer rows
 * [fbRowBegin, fbRowBegin + fbRowCount).  Per-pixel device buffers handed to the band entry points (linear
 * depth, surface planes, radiance) hold exactly those rows, first row = fbRowBegin.  The whole frame is the
 * band {0, Ty, 0, H}; use sailor_hip_band_whole_frame / sailor_hip_band_for_rank to fill one.
 */
typedef struct SailorBand {
    int32_t tileRowBegin;
    int32_t tileRowEnd;
    int32_t fbRowBegin;
    int32_t fbRowCount;
} SailorBand;

typedef struct SailorHipContext SailorHipContext; /* opaque */

/* ---- library / context --------------------------------------------------------------------------------- */

SAILOR_HIP_API int sailor_hip_version(void);                 /* 1000*major + minor */
SAILOR_HIP_API const char* sailor_hip_status_string(int status);
SAILOR_HIP_API int sailor_hip_device_count(int* outCount);

/* Replaces: RHI/Renderer.cpp:60-63 (backend instantiation) + IGraphicsDriver::Initialize (RHI/GraphicsDriver.h:63).
 * flags = 0: record on `stream`, a hipStream_t the caller owns (NULL = the device's default stream, which is what
 * torch.cuda.current_stream() is unless the caller switched streams).  flags = SAILOR_CTX_OWN_STREAM: `stream` is
 * ignored and the context creates (and owns) a non-blocking stream -- the graphics-queue analogue of the reference. */
#define SAILOR_CTX_OWN_STREAM 1u
SAILOR_HIP_API int sailor_hip_context_create(int deviceOrdinal, void* stream, uint32_t flags, SailorHipContext** outContext);
SAILOR_HIP_API int sailor_hip_context_destroy(SailorHipContext* ctx);
/* Replaces: IGraphicsDriver::WaitIdle (RHI/GraphicsDriver.h:83) */
SAILOR_HIP_API int sailor_hip_context_synchronize(SailorHipContext* ctx);
SAILOR_HIP_API int sailor_hip_context_stream(SailorHipContext* ctx, void** outStream);
/* Text of the last HIP/RCCL error seen by this context (never NULL). */
SAILOR_HIP_API const char* sailor_hip_context_last_error(SailorHipContext* ctx);

/* Orders two contexts of one device: everything recorded on `waiter` after this call starts after everything recorded on `signaller` before it
 * (an event on the signaller's stream, a wait on the waiter's: the Vulkan backend's semaphore between two queues, VulkanGraphicsDriver.cpp
 * SubmitCommandList's wait / signal lists).  Used by the HIP backend to run the cull's compaction step beside the shade (SAILOR_CULL_DEFER_PACK). */
SAILOR_HIP_API int sailor_hip_context_wait_for(SailorHipContext* waiter, SailorHipContext* signaller);

/* Measurement aid (no reference counterpart): the next `count` kernel launches recorded through this context carry a HIP event pair on their own
 * dispatch packets (hipExtLaunchKernel's start / stop events) in slots [firstSlot, firstSlot + count), in launch order -- e.g. the four kernels of
 * one sailor_hip_light_cull, or the one of a sailor_hip_shade.  sailor_hip_context_timed_launch_ms waits for a slot's kernel and returns its
 * duration: the command processor's timestamps of THAT kernel -- the figure rocprofv3 --kernel-trace reports -- without draining the stream around
 * it as events recorded in front of and behind a launch do.  Eager launches only (not inside a hipGraph capture); at most 4 096 slots. */
SAILOR_HIP_API int sailor_hip_context_time_launches(SailorHipContext* ctx, int32_t firstSlot, int32_t count);
SAILOR_HIP_API int sailor_hip_context_timed_launch_ms(SailorHipContext* ctx, int32_t slot, float* outMs);
/* Measurement aid (no reference counterpart): *outCount = the number of kernels the path's entry points have launched through this context since it was
 * created (exactly the launches that take a timing slot above); outNames[0 .. n) = the names of the last n = min(maxNames, 16, *outCount) of them,
 * oldest first (static strings; further entries NULL).  A caller that wants the kernels of ONE call reads the count in front of and behind it -- which
 * kernels a cull chain consists of (the band selection's two kernels or not, the wide list builder or not, brute force) is the library's decision, not the caller's guess.
 * sailor_hip_context_time_launches is refused (SAILOR_HIP_ERR_UNSUPPORTED) while the context's stream is being captured into a hipGraph. */
SAILOR_HIP_API int sailor_hip_context_launch_log(SailorHipContext* ctx, uint64_t* outCount, const char** outNames, int32_t maxNames);
/* Measurement aid (no reference counterpart): one float4-per-lane streaming copy of `bytes` (a multiple of 16; both pointers 16-byte aligned) from dSrc to
 * dDst on the context's stream -- the yardstick of THIS box and process for the roofline figures (2 x bytes of HBM traffic per call; time it with
 * sailor_hip_context_time_launches like any kernel of the path).  Boxes of the pool differ by +-5 %; the guide's 6.29 TB/s is one of them. */
SAILOR_HIP_API int sailor_hip_copy_probe(SailorHipContext* ctx, const void* dSrc, void* dDst, size_t bytes);
/* Measurement aid (no reference counterpart): an empty one-wave kernel on the context's stream.  A kernel's dispatch-packet timestamps begin when its packet is
 * taken up and so include the wait for its predecessor's last blocks; a marker in front of a kernel takes that wait onto its own reading. */
SAILOR_HIP_API int sailor_hip_marker(SailorHipContext* ctx);

/* ---- buffers: IGraphicsDriver::CreateBuffer (RHI/GraphicsDriver.h:89-90), AddSsboToShaderBindings (:154),
 *      IGraphicsDriverCommands::UpdateShaderBinding / UpdateBuffer (:303-304) -------------------------------- */
SAILOR_HIP_API int sailor_hip_buffer_create(SailorHipContext* ctx, size_t bytes, void** outDevicePtr);
SAILOR_HIP_API int sailor_hip_buffer_free(SailorHipContext* ctx, void* devicePtr);
/* async host->device copy on the context stream; `src` bytes are staged at record time (the reference copies
 * push-constant / update payloads at record time too: VulkanCommandBuffer.cpp:679-685) */
SAILOR_HIP_API int sailor_hip_buffer_upload(SailorHipContext* ctx, void* dstDevice, size_t dstOffset, const void* src, size_t bytes);
/* synchronous device->host copy (waits for the stream) */
SAILOR_HIP_API int sailor_hip_buffer_download(SailorHipContext* ctx, void* dstHost, const void* srcDevice, size_t srcOffset, size_t bytes);
/* device-to-device copy on the context's stream (the BlitImage of equally sized images, e.g. EnvironmentNode.cpp:200-203) */
SAILOR_HIP_API int sailor_hip_buffer_copy(SailorHipContext* ctx, void* dstDevice, size_t dstOffset, const void* srcDevice, size_t srcOffset, size_t bytes);
SAILOR_HIP_API int sailor_hip_buffer_fill_u32(SailorHipContext* ctx, void* dstDevice, size_t dstOffset, uint32_t value, size_t count);
/* `count` records of `wordsPerRecord` (1 .. 4) words each, every record = value[0 .. wordsPerRecord): IGraphicsDriverCommands::ClearImage (:294) of a target
 * with more than one channel to a colour whose channels differ (ClearNode.cpp:104-106) */
SAILOR_HIP_API int sailor_hip_buffer_fill_pattern(SailorHipContext* ctx, void* dstDevice, size_t dstOffset, const uint32_t* value, uint32_t wordsPerRecord,
                                                  size_t count);

/* ---- bands ---------------------------------------------------------------------------------------------- */
SAILOR_HIP_API int sailor_hip_num_tiles(int32_t width, int32_t height, int32_t* outTilesX, int32_t* outTilesY); /* LightCullingNode.cpp:56-57 */
SAILOR_HIP_API int sailor_hip_band_whole_frame(int32_t width, int32_t height, SailorBand* outBand);
/* an arbitrary contiguous run of tile rows [tileRowBegin, tileRowEnd) -- for cost-balanced partitions */
SAILOR_HIP_API int sailor_hip_band_from_tile_rows(int32_t width, int32_t height, int32_t tileRowBegin, int32_t tileRowEnd, SailorBand* outBand);
/* contiguous tile-row bands: rank g of G gets rows [floor(g*Ty/G), floor((g+1)*Ty/G)) */
SAILOR_HIP_API int sailor_hip_band_for_rank(int32_t width, int32_t height, int32_t rank, int32_t worldSize, SailorBand* outBand);
/* 1 if `band` is a run of whole tile rows of a width x height frame with the matching framebuffer rows (what the three helpers above
 * produce), else 0.  Every band entry point refuses anything else. */
SAILOR_HIP_API int sailor_hip_band_is_valid(int32_t width, int32_t height, const SailorBand* band);

/* ---- K0 + K1: tile light cull ---------------------------------------------------------------------------
 * Replaces: the Dispatch recorded by LightCullingNode::Process (FrameGraph/LightCullingNode.cpp:74-77) and the
 * whole of Content/Shaders/ComputeLightCulling.shader, under the canonical sequential semantics of SURVEY.md
 * Appendix A (ascending-light-index candidates, first 196, nearest-128 selection, prefix-sum offsets).
 *
 *   frame, pc      : host structs, copied at record time
 *   dLights        : device, pc->lightsNum x SailorLightShaderData (binding set 0 / binding 0 `light`)
 *   dLinearDepth   : device, R32F linear depth rows of `band` (binding set 1 / binding 2 `sceneDepth`)
 *   dLightsGrid    : device out, one SailorLightsGrid per tile OF THE BAND (band-local tile index
 *                    (ty - tileRowBegin)*Tx + tx); offset is band-local: 1 + sum of num over earlier band tiles
 *   dCulledLights  : device out, uint32: [0] = sum of num over the band, [offset+i] = i-th light of the tile;
 *                    capacity culledCapacity uints: 1 + bandTiles*128 holds every possible result.  The reference allocates
 *                    bandTiles*128 (one short, LightCullingNode.cpp:64): that size is accepted, and a list that does not
 *                    fit is cut -- lightsGrid[tile].num and [0] then say what was written, so a consumer never reads past
 *                    the buffer; anything smaller is SAILOR_HIP_ERR_INVALID_ARGUMENT
 *   dWorkspace     : device scratch of at least sailor_hip_light_cull_workspace_size(...) bytes
 *   flags          : SAILOR_CULL_* bits
 * For the whole-frame band the outputs ARE the reference's `lightsGrid` / `culledLights` buffers.
 */
#define SAILOR_CULL_DEFAULT 0u
#define SAILOR_CULL_BRUTE_FORCE 1u /* skip the conservative macro-tile pre-filter (same results, for validation) */
#define SAILOR_CULL_RAW_DEPTH 2u   /* dLinearDepth holds the RAW reversed-Z depth attachment: the depth pass linearises it on
                                      the fly (sailor_hip_linearize_depth's arithmetic, same bits) -- the LinearizeDepth node's
                                      full-screen pass and its 8 bytes per pixel disappear.  x -> zNear / x is monotone, so
                                      the tile's min / max are taken on the raw bits and only two values per tile are divided */
#define SAILOR_CULL_INTERVAL_MASKS 4u /* build the pre-filter masks from per-light band intervals (the default above 262 144 lights) also for small
                                       * light sets with <= 256 bands: same lists, for validation */
#define SAILOR_CULL_DEFER_PACK 8u     /* stop after the per-tile lists: dLightsGrid / dCulledLights are NOT written by this call.  The lists are complete in the
                                       * workspace (sailor_hip_light_cull_tile_lists; sailor_hip_shade_tile_lists shades from them), and
                                       * sailor_hip_light_cull_pack -- on any context / stream ordered after this call, e.g. a second stream beside the shade --
                                       * produces the two canonical buffers from them, bit for bit what the undeferred call writes */

#define SAILOR_CULL_PREPARE_LIGHTS 16u /* sailor_hip_light_cull_prepared only: EVERY light is dirty this frame (LightingECS::Tick re-uploaded the whole set,
                                        * ECS/LightingECS.cpp:152-191).  The cull's per-light pass reads the 112-byte records in dLights and WRITES the prepared
                                        * views of all pc->lightsNum lights into dPreparedLights on the way -- sailor_hip_prepare_lights(0, lightsNum) folded
                                        * into the cull: one pass over the records instead of two, one launch less; the same bits in the views, the same lists */
#define SAILOR_CULL_BAND_SELECT 32u    /* a band of a split frame: select the lights that can reach the band's rows first (k0_band_count + k0_band_scatter: an ordered compaction on the band's
                                        * top / bottom planes) and run the chain on those -- the default from 131 072 lights on; this flag forces it for smaller sets
                                        * (same lists bit for bit; validation) */
#define SAILOR_CULL_NO_BAND_SELECT 64u /* ... never (same lists; A / B) */
#define SAILOR_CULL_PREPARE_SELECTED 128u /* with SAILOR_CULL_PREPARE_LIGHTS on a band whose lights are selected (above): the staged SHADE records are derived only for
                                        * the selected lights -- all this band's shade of THIS frame can read -- instead of for all of them (the 20-byte cull views
                                        * still for all).  For hosts that re-prepare every frame (every light dirty every frame): a record of a light outside the
                                        * selection keeps whatever an earlier call left there, so a later frame that culls WITHOUT re-preparing must not follow.
                                        * Ignored where no selection runs */
SAILOR_HIP_API size_t sailor_hip_light_cull_workspace_size(int32_t width, int32_t height, int32_t lightsCapacity, const SailorBand* band);
SAILOR_HIP_API int sailor_hip_light_cull(SailorHipContext* ctx,
                                         const SailorUboFrameData* frame, const SailorLightCullPushConstants* pc,
                                         const SailorLightShaderData* dLights, const float* dLinearDepth,
                                         SailorLightsGrid* dLightsGrid, uint32_t* dCulledLights, size_t culledCapacity,
                                         void* dWorkspace, size_t workspaceBytes,
                                         const SailorBand* band, uint32_t flags);

/* The cull's own per-tile form of the lists (round 4).  Every tile of the band leaves its list in a fixed 128-entry slot of the workspace --
 * tileLists[bandTile * 128 + i] = i-th light of the tile, the same entries in the same order as culledLights[offset + i] -- and its length (<= 128) in
 * tileNum[bandTile].  A consumer that only needs "the lights of tile t" (the shade: Standard.shader:422-436) reads them there and does not depend on the
 * compaction into the reference's layout, which then leaves the frame's critical path: SAILOR_CULL_DEFER_PACK + sailor_hip_light_cull_pack on a
 * second stream.  The pointers depend on (width, height, band) alone (lightsCapacity: any light count the workspace can hold) and stay valid until the
 * next cull on the same workspace.  The band shade's hint below (the lengths as bytes) is written by k1_tile_cull as well: it is there with a deferred
 * pack too, so a band's shade does not wait for the compaction either. */
SAILOR_HIP_API int sailor_hip_light_cull_tile_lists(int32_t width, int32_t height, int32_t lightsCapacity, const SailorBand* band, const void* dWorkspace,
                                                    const uint32_t** outTileNum, const uint32_t** outTileLists);
/* Replaces: nothing of its own -- the second half of the Dispatch at LightCullingNode.cpp:74-77 (Appendix A step 6: offsets = prefix sum of the list
 * lengths in tile order, ComputeLightCulling.shader:227-238 without its atomic allocation order) when sailor_hip_light_cull ran with
 * SAILOR_CULL_DEFER_PACK.  Arguments as there. */
SAILOR_HIP_API int sailor_hip_light_cull_pack(SailorHipContext* ctx, int32_t width, int32_t height, int32_t lightsCapacity, const SailorBand* band,
                                              const void* dWorkspace, SailorLightsGrid* dLightsGrid, uint32_t* dCulledLights, size_t culledCapacity);

/* Shading hint of a band.  A band of a split frame is a round or two of blocks, so its longest tile is its duration, and a tile in the middle of a light
 * cluster keeps one block busy ~100x longer than an average one.  This returns the band's per-tile list lengths as BYTES (T bytes, tile order, <= 128 each;
 * every sailor_hip_light_cull writes them beside tileNum -- nothing extra, no atomics: round 4's form, a list of the long tiles appended through two
 * device-scope counters, cost the cull up to 12.7 us on half a 4K frame).  Handing the pointer to sailor_hip_shade_ex (band smaller than the frame, no
 * ambient term; with or without shadow maps) switches the BAND FORM of the launch on: the tiles with at least `splitMin` lights -- 64 on a band of up to
 * 12 000 tiles, 96 on a larger one; SAILOR_SPLIT_MIN=<1..128> overrides for A / B runs -- go to "split" blocks -- one per (tile, 8x8
 * quadrant), four waves sharing the quadrant's list -- at the front of the grid, which find them in these bytes.  Lists and every tile below the threshold keep
 * their bits; a split tile's radiance differs from the one-block form by the order of four partial sums per pixel (within the shade tolerance).  With the
 * ambient term the pointer is ignored.  NULL for the whole-frame band (on the whole frame the split measured no gain), for a band of more than 12 000
 * tiles when lightsCapacity >= 131 072 (short lists, no long tiles to split: the whole frame's launch form pipelines better there) and on bad arguments.  Valid until
 * the next sailor_hip_light_cull on the same workspace.  `lightsCapacity` only has to be a light count the workspace can hold: the bytes' place in the
 * workspace depends on (width, height, band) alone.  (The return type is kept from round 2's word array; the data are bytes.) */
SAILOR_HIP_API const uint32_t* sailor_hip_light_cull_tile_order(int32_t width, int32_t height, int32_t lightsCapacity, const SailorBand* band,
                                                                const void* dWorkspace);

/* ---- LinearizeDepth: the pass immediately before K1 ---------------------------------------
 * Replaces: the full-screen draw of LinearizeDepthNode::Process (FrameGraph/LinearizeDepthNode.cpp:22-109) with the
 * fragment shader Content/Shaders/LinearizeDepth.shader:61-73 under its REVERSE_Z_INF_FAR_PLANE define (:6):
 *   linearDepth = -frame.cameraZNearZFar.x / depth;  outColor = vec4(-linearDepth)
 * i.e. out = zNear / raw with one IEEE division (both negations are exact).  The quad's flipped texcoord (:49) and the
 * driver's flipped viewport (GraphicsDriver/Vulkan/VulkanDevice.cpp:681) cancel: output row r reads depth row r.
 *   dRawDepth / dLinearDepth : device, float32, `rows` x `width`, row-major (any contiguous run of framebuffer rows)
 * raw = 0 (nothing drawn, far plane at infinity) gives +inf, as in the reference.
 */
SAILOR_HIP_API int sailor_hip_linearize_depth(SailorHipContext* ctx, const SailorUboFrameData* frame,
                                              const float* dRawDepth, float* dLinearDepth, int32_t width, int32_t rows);

/* Tuning diagnostics (synchronises): out8 = {numBands, mask bits set, numGroups, sum of group list lengths, overflowed
 * groups, longest group list, 64-bit words per band, bits set in the column masks} for the intermediate pre-filter state
 * left in dWorkspace by the last sailor_hip_light_cull of the same geometry. */
/* ---- prepared lights: the per-light half of the path, run where the `light` SSBO is WRITTEN instead of where it is read ------------------
 * The reference re-derives everything per light inside its per-tile / per-fragment loops.  Lights change when LightingECS::Tick uploads a dirty run
 * (ECS/LightingECS.cpp:182-191 -> IGraphicsDriverCommands::UpdateShaderBinding, RHI/GraphicsDriver.h:303), not every frame, so the HIP backend derives
 * two views of the records right behind that copy ("pre-split SoA"), for the lights [firstLight, firstLight + count) it carried:
 *   - the cull's view: (worldPosition, bounds.x) as one float4 and the type, dense arrays -- 20 bytes per light for k01_prepare to stream each frame
 *     instead of 112;
 *   - the shade's staged record, 80 bytes: normalised spot axis, reach threshold, 1 / bounds.x, the "every parameter is finite" bit ... -- what every
 *     shade block otherwise derives again for every slot of its tile's list.
 * dPrepared is caller-owned device memory of sailor_hip_prepared_lights_size(lightsCapacity) bytes, 16-byte aligned; lightsCapacity fixes its layout
 * and must be the same in every call that names the buffer.  sailor_hip_light_cull_prepared / sailor_hip_shade_prepared take it beside dLights (NULL =
 * the entry points above: same lists, same radiance, bit for bit -- the kernels run the same instructions on the same inputs, only elsewhere).
 * The caller keeps it in step with dLights: a record changed without a prepare of its slot is a stale light, as a missed upload would be. */
SAILOR_HIP_API size_t sailor_hip_prepared_lights_size(int32_t lightsCapacity);
SAILOR_HIP_API int sailor_hip_prepare_lights(SailorHipContext* ctx, const SailorLightShaderData* dLights, int32_t firstLight, int32_t count,
                                             int32_t lightsCapacity, void* dPrepared, size_t preparedBytes);
/* the three arrays inside dPrepared (float4 posRadius[capacity]; uint32 type[capacity]; float4 staged[capacity][5]); any out pointer may be NULL */
SAILOR_HIP_API int sailor_hip_prepared_lights_views(int32_t lightsCapacity, const void* dPrepared, const void** outPosRadius, const void** outType,
                                                    const void** outStaged);
SAILOR_HIP_API int sailor_hip_light_cull_prepared(SailorHipContext* ctx,
                                                  const SailorUboFrameData* frame, const SailorLightCullPushConstants* pc,
                                                  const SailorLightShaderData* dLights, const float* dLinearDepth,
                                                  SailorLightsGrid* dLightsGrid, uint32_t* dCulledLights, size_t culledCapacity,
                                                  void* dWorkspace, size_t workspaceBytes,
                                                  const SailorBand* band, uint32_t flags,
                                                  const void* dPreparedLights /* or NULL */, int32_t preparedCapacity);
SAILOR_HIP_API int sailor_hip_light_cull_diagnostics(SailorHipContext* ctx, int32_t width, int32_t height, int32_t lightsNum, const SailorBand* band,
                                                     const void* dWorkspace, uint64_t* out8);
/* The band-local light selection (SAILOR_CULL_BAND_SELECT and its default above) as the last cull with this geometry and pc->lightsNum == lightsNum left
 * it in dWorkspace: *outSelectedCount -> one device uint32, the number M of lights that can reach the band; *outLightMap -> M device uint32, the
 * selected lights' indices in ascending order.  Meaningful only if that cull ran the selection (sailor_hip_context_launch_log names a call's kernels:
 * "k0_band_count", "k0_band_scatter" are the first two of the chain then).  Tests and diagnostics; either out pointer may be NULL. */
SAILOR_HIP_API int sailor_hip_light_cull_band_selection(int32_t width, int32_t height, int32_t lightsNum, const SailorBand* band, const void* dWorkspace,
                                                        const uint32_t** outSelectedCount, const uint32_t** outLightMap);

/* Multi-GPU stitch helpers.  After an all-gather of the per-band totals, rebase a band's grid
 * to the canonical global offsets: offset += globalBase (globalBase = sum of num over all earlier bands). */
SAILOR_HIP_API int sailor_hip_light_grid_rebase(SailorHipContext* ctx, SailorLightsGrid* dLightsGrid, int32_t numTiles, uint32_t globalBase);

/* ---- K2 + K3: PBR shade over per-tile light lists, with CSM sampling --------------------------------------
 * Replaces: the fragment work of Content/Shaders/Standard.shader main() (:377-439) + CalculateLighting (:259-341)
 * + Lighting.glsl:39-76,168-284 for the draws recorded by RenderSceneNode::Process (FrameGraph/RenderSceneNode.cpp:109),
 * executed as compute over a surface buffer instead of rasterised fragments (ambient/IBL term == 0).
 *
 *   dSurface       : device, 3 planes of float4 per pixel, plane-major, each plane = band rows x width:
 *                    P0 = (worldPos.xyz, albedo.a)  P1 = (normal.xyz, roughness)  P2 = (albedo.rgb, metallic)
 *   surfacePlaneStride : distance between planes in float4 elements (>= band rows * width)
 *   dLightsGrid / dCulledLights : the lists of the SAME band as produced by sailor_hip_light_cull (band-local)
 *   csm            : host struct or NULL (no directional shadowing: factor 1)
 *   dRadiance      : device out, float4 per pixel of the band (rgb = sum over lights, a = albedo.a)
 */
SAILOR_HIP_API int sailor_hip_shade(SailorHipContext* ctx, const SailorUboFrameData* frame,
                                    const float* dSurface, size_t surfacePlaneStride,
                                    const SailorLightShaderData* dLights, int32_t lightsNum,
                                    const SailorLightsGrid* dLightsGrid, const uint32_t* dCulledLights,
                                    const SailorCsmDesc* csm, float* dRadiance,
                                    const SailorBand* band);

/* As sailor_hip_shade, plus the ambient term: outColor.rgb = AmbientLighting(...) + sum over lights
 * (Standard.shader:425).  ibl == NULL and dTileOrder == NULL is sailor_hip_shade. */
SAILOR_HIP_API int sailor_hip_shade_ex(SailorHipContext* ctx, const SailorUboFrameData* frame,
                                       const float* dSurface, size_t surfacePlaneStride,
                                       const SailorLightShaderData* dLights, int32_t lightsNum,
                                       const SailorLightsGrid* dLightsGrid, const uint32_t* dCulledLights,
                                       const SailorCsmDesc* csm, const SailorIblDesc* ibl, float* dRadiance,
                                       const SailorBand* band, const uint32_t* dTileOrder /* sailor_hip_light_cull_tile_order or NULL */);

/* As sailor_hip_shade_ex with the lights' staged records (sailor_hip_prepare_lights, above); dPreparedLights == NULL is sailor_hip_shade_ex.
 * With it dLights is not read and may be NULL. */
SAILOR_HIP_API int sailor_hip_shade_prepared(SailorHipContext* ctx, const SailorUboFrameData* frame,
                                             const float* dSurface, size_t surfacePlaneStride,
                                             const SailorLightShaderData* dLights, int32_t lightsNum,
                                             const SailorLightsGrid* dLightsGrid, const uint32_t* dCulledLights,
                                             const SailorCsmDesc* csm, const SailorIblDesc* ibl, float* dRadiance,
                                             const SailorBand* band, const uint32_t* dTileOrder,
                                             const void* dPreparedLights /* or NULL */, int32_t preparedCapacity);

/* As sailor_hip_shade_prepared, reading the lists where the cull left them (sailor_hip_light_cull_tile_lists: dTileNum[t] entries at
 * dTileLists[128 t ..] for band tile t) instead of through lightsGrid / culledLights: the same entries in the same order, hence the same radiance bit
 * for bit -- and no dependence on the compaction step (SAILOR_CULL_DEFER_PACK).  This is the form the HIP backend records for RenderSceneNode's
 * draws when the lists come from its own LightCulling node (Standard.shader:422-436 is the loop it replaces either way). */
SAILOR_HIP_API int sailor_hip_shade_tile_lists(SailorHipContext* ctx, const SailorUboFrameData* frame,
                                               const float* dSurface, size_t surfacePlaneStride,
                                               const SailorLightShaderData* dLights, int32_t lightsNum,
                                               const uint32_t* dTileNum, const uint32_t* dTileLists,
                                               const SailorCsmDesc* csm, const SailorIblDesc* ibl, float* dRadiance,
                                               const SailorBand* band, const uint32_t* dTileOrder,
                                               const void* dPreparedLights /* or NULL */, int32_t preparedCapacity);

/* Self-check of the shade kernels' short forms of exact arithmetic (no reference counterpart: the shader leaves sqrt and 1 / x to the driver).
 * K2 evaluates normalize() as v * (1 / sqrt(dot(v, v))) with a correctly rounded square root and reciprocal, but not through the compiler's
 * 21- and 12-instruction expansions: sqrt as one Newton step on v_rsq_f32 for x in [2^-96, inf), 1 / s as one Newton step on v_rcp_f32 for
 * |s| in [2^-126, 2^126] (sailor_amd/csrc/shade_body.h: sqrt_exact, rcp_of_sqrt).  This runs both against sqrtf and 1.0f / s over EVERY float of
 * those ranges on the device the context is bound to (about a second) and writes the number of inputs whose bits differ:
 *   mismatches[0] = square root, mismatches[1] = reciprocal.  The quotient from a staged reciprocal (div_stored: Markstein's correction step,
 * exact by theorem when nothing over- or underflows) has 2^64 operand pairs; 2^30 pseudo-random ones in the ranges its callers guarantee are
 * compared with the IEEE division: mismatches[2].  All three must be 0; dScratch: device, 24 bytes. */
SAILOR_HIP_API int sailor_hip_self_check_exact_math(SailorHipContext* ctx, void* dScratch, uint64_t mismatches[3]);

/* The split-sum BRDF look-up table sampled by AmbientLighting: Content/Shaders/ComputeBrdfLut.shader:26-71 (1 024 Hammersley /
 * GGX samples per texel), dispatched once at start-up.  dLut: device, height x width float2 (the reference image is RG16F). */
SAILOR_HIP_API int sailor_hip_compute_brdf_lut(SailorHipContext* ctx, float* dLut, int32_t width, int32_t height);

/* Replaces: IGraphicsDriverCommands::ConvertEquirect2Cubemap (GraphicsDriver/Vulkan/VulkanGraphicsDriver.cpp:1662-1686) =
 * Content/Shaders/ComputeEquirect2Cube.shader:20-58, the first step of the raw environment cube (FrameGraph/EnvironmentNode.cpp:131-135).
 *   dEquirect : device in, eqWidth x eqHeight RGBA32F ("src"), rows top to bottom; `repeat` != 0 = the texture's sampler wraps
 *               (TextureAssetInfo.h:30 default), 0 = clamp-to-edge
 *   dCube     : device out, 6 x size x size RGBA32F = level 0 of the cube chain ("dst"; the reference image is RGBA16F)
 *   coverWidth / coverHeight : the reference dispatches equirectExtent / 32 groups (not cubeSize / 32), so only texels with
 *               x < coverWidth and y < coverHeight are written; pass `size` twice for the whole cube */
SAILOR_HIP_API int sailor_hip_equirect_to_cube(SailorHipContext* ctx, const float* dEquirect, int32_t eqWidth, int32_t eqHeight, int32_t repeat,
                                               float* dCube, int32_t size, int32_t coverWidth, int32_t coverHeight);
/* Replaces: IGraphicsDriverCommands::GenerateMipMaps on a cubemap (GraphicsDriver/Vulkan/VulkanCommandBuffer.cpp:814-907; called at
 * EnvironmentNode.cpp:137): level i = a 2:1 VK_FILTER_LINEAR blit of level i - 1, face by face = the mean of 2 x 2 texels.
 *   dCube : device in/out, the level-major RGBA32F chain; level 0 is read, levels 1 .. levels-1 are written */
SAILOR_HIP_API int sailor_hip_generate_mipmaps_cube(SailorHipContext* ctx, float* dCube, int32_t size, int32_t levels);

/* Replaces: Content/Shaders/ComputeIrradianceMap.shader:78-101 for the Dispatch at FrameGraph/EnvironmentNode.cpp:264-269
 * (IrradianceMapSize / 32 groups squared x 6): 65 536 uniform hemisphere samples per texel of the environment cube at lod 0.
 *   dEnv        : device in, RGBA32F cube mip chain ("envMap"): level-major, then face (+X -X +Y -Y +Z -Z), then rows of texels
 *   dIrradiance : device out, 6 x size x size RGBA32F ("irradianceMap"; the reference image is RGBA16F), alpha = 1 */
SAILOR_HIP_API int sailor_hip_compute_irradiance_map(SailorHipContext* ctx, const float* dEnv, int32_t envSize, int32_t envLevels,
                                                     float* dIrradiance, int32_t size);

/* Replaces: the "pre-filter the mip chain" section of FrameGraph/EnvironmentNode.cpp:196-233 -- level 0 copied from the raw cube (:200-203),
 * level l = 1 .. levels-1 by Content/Shaders/ComputeEnvMap_IBL.shader:76-136 with push constants { level - 1, roughness = l / (levels - 1) }:
 * 1 024 GGX importance samples per texel, mip-filtered lookups into all levels of the raw cube.
 *   dRawEnv : device in, RGBA32F cube mip chain ("rawEnvMap", size x size x 6, `levels` levels, layout as above)
 *   dEnv    : device out, the same layout ("envMap[]"); must not alias dRawEnv */
SAILOR_HIP_API int sailor_hip_prefilter_env_map(SailorHipContext* ctx, const float* dRawEnv, float* dEnv, int32_t size, int32_t levels);
/* One Dispatch of that loop (EnvironmentNode.cpp:223-231): output mip `level` (the shader's push constant is level - 1) at `roughness`. */
SAILOR_HIP_API int sailor_hip_prefilter_env_level(SailorHipContext* ctx, const float* dRawEnv, float* dEnv, int32_t size, int32_t levels,
                                                  int32_t level, float roughness);

/* ---- EVSM shadow-map blur ---------------------------------------------------------------
 * Replaces: the two full-screen draws "Blur Horizontal" / "Blur Vertical" of ShadowPrepassNode::Process
 * (FrameGraph/ShadowPrepassNode.cpp:283-356) with Content/Shaders/Blur.shader (defines EVSM + HORIZONTAL | VERTICAL, :66-98) ->
 * GaussianBlur_Evsm (Lighting.glsl:83-127) over the cascade-0 moments map (RGBA32F): .zw blurred with the umbra radius, .xy with
 * the penumbra radius (RHI/SceneView.h:60; ECS/LightingECS.h:68 ShadowCascadeBlur = (2, 5) for cascade 0), radii capped at 12.
 *   dMap  : device, height x width float4, blurred IN PLACE (the node renders into a temporary target and back)
 *   dTemp : device scratch of the same size (the node's blurAttachment)
 * Taps sit on texel centres: the texel itself, clamp-to-edge.  Same sums in the same order as the shader: bit-exact vs the oracle. */
SAILOR_HIP_API int sailor_hip_evsm_blur(SailorHipContext* ctx, float* dMap, float* dTemp, int32_t width, int32_t height,
                                        int32_t radiusUmbra, int32_t radiusPenumbra);
/* one of the two draws: vertical == 0 is Blur.shader with HORIZONTAL (texelSize.y = 0, :72-74), else VERTICAL (:68-70) */
SAILOR_HIP_API int sailor_hip_evsm_blur_pass(SailorHipContext* ctx, const float* dSrc, float* dDst, int32_t width, int32_t height,
                                             int32_t radiusUmbra, int32_t radiusPenumbra, int32_t vertical);

/* ---- K4: ECS transform + bounds + frustum-cull sweep -------------------------------------------------------
 * Replaces: TransformECS::Tick full-sweep branch + CalculateMatrices (ECS/TransformECS.cpp:144-212),
 * Transform::Matrix (Math/Transform.cpp:39-42), the AABB::Apply of StaticMeshRendererECS::Tick
 * (ECS/StaticMeshRendererECS.cpp:40-58, Math/Bounds.cpp:479-492) and the Frustum::OverlapsAABB sweep that
 * RHISceneView::TraceScene performs through the octree (RHI/SceneView.cpp:56, Math/Bounds.cpp:245-260), over flat
 * level-sorted arrays.
 *
 *   entities are level-sorted: levelOffsets[l]..levelOffsets[l+1] is hierarchy level l (host array of
 *   numLevels+1 entries), dParent[i] = index of the parent (in an earlier level) or 0xFFFFFFFF for roots
 *   planes         : host, 6 x vec4 (L,R,T,B,N,F) from sailor_host_extract_frustum_planes
 *   dWorld         : device out, mat4 per entity (m_cachedWorldMatrix)
 *   dWorldAabb     : device out, SailorAABB per entity
 *   dVisibility    : device out, 1 bit per entity, LSB-first in uint64 words, ceil(n/64) words
 */
SAILOR_HIP_API int sailor_hip_ecs_sweep(SailorHipContext* ctx, uint32_t numEntities,
                                        const SailorTransform* dTransforms, const uint32_t* dParent,
                                        const uint32_t* levelOffsets, uint32_t numLevels,
                                        const SailorAABB* dLocalAabb, const float* planes,
                                        float* dWorld, SailorAABB* dWorldAabb, uint64_t* dVisibility);
/* K4 split across the ranks of a node (the reference fans the same sweep out in 1 024-entity chunks over its worker threads,
 * ECS/StaticMeshRendererECS.cpp:17-150): the sweep of the slice [entityBegin, entityEnd) of the entity array only -- its entries of dWorld / dWorldAabb,
 * its bits of dVisibility.  A hierarchy of at most four levels (the one-launch form: an entity rebuilds its ancestors' relative matrices from their TRS
 * records, the same bits as the level-by-level product) takes ANY slice and needs nothing another rank computes; a deeper one reads its parents' world
 * matrices and is refused unless the slice is the whole set (SAILOR_HIP_ERR_UNSUPPORTED: sweep it replicated).
 * sailor_hip_ecs_range_for_rank: rank r's slice of an equal split in whole 64-entity visibility words, ceil(words / worldSize) = *outWordsPerRank per
 * rank (the last ranks may get fewer entities, or none).  sailor_hip_exchange_visibility: ONE in-place ncclAllGather of those words on `comm` and the
 * context's stream -- dVisibility must hold worldSize * wordsPerRank uint64, which is MORE than sailor_hip_ecs_sweep's ceil(n / 64) when the words do
 * not divide evenly (n = 100 on 8 ranks: 8 words, not 2); `visibilityWords` is the buffer's capacity in uint64 and a smaller one is refused
 * (SAILOR_HIP_ERR_INVALID_ARGUMENT) instead of overrun -- after which every rank holds the whole bitmask (C5: 128 KB).  World
 * matrices and boxes stay where they were computed: a consumer that needs ALL of them on every rank (instance data for draws) is better served by the
 * replicated sweep -- 64 B + 24 B per entity over xGMI cost more than the 38 us the whole sweep takes on one GPU. */
SAILOR_HIP_API int sailor_hip_ecs_sweep_range(SailorHipContext* ctx, uint32_t numEntities,
                                              const SailorTransform* dTransforms, const uint32_t* dParent,
                                              const uint32_t* levelOffsets, uint32_t numLevels,
                                              const SailorAABB* dLocalAabb, const float* planes,
                                              float* dWorld, SailorAABB* dWorldAabb, uint64_t* dVisibility,
                                              uint32_t entityBegin, uint32_t entityEnd);
/* Row E4 as the reference runs it: RHISceneView::TraceScene (RHI/SceneView.cpp:56, the camera snapshot at :170, the cascade mesh lists at
 * ECS/LightingECS.cpp:296) walks a TOctree whose elements are the world boxes TRUNCATED to integers -- StaticMeshRendererECS.cpp:81,96,132 pass
 * GetCenter() / GetExtents() (Math/Bounds.cpp:455-463) to TOctree::Update(const glm::ivec3&, const glm::ivec3&, ...) -- and draws only what the
 * root (ivec3(0), RHI/SceneView.h:91-92) STRICTLY contains (Containers/Octree.h:44-53: -h < p - e and h > p + e per axis, h = rootSize / 2 as an
 * integer), traced with Frustum::OverlapsAABB on AABB((vec3)p, (vec3)e) (Octree.h:239-274) once the root's own box passes (:239-247).
 * sailor_hip_ecs_sweep and sailor_hip_csm_caster_masks test the float boxes flat (SAILOR_TRACE_FLAT_FLOAT_BOXES); SAILOR_TRACE_OCTREE_INT_BOXES
 * gives the reference's set without building a tree: per entity, inserted = the root strictly contains the integer box, visible =
 * inserted, the root's box passes and the integer box passes.  That is the walk's answer, bit for bit, whenever every truncated extent is >= 0 --
 * always so for the sweep's own world boxes (AABB::Apply yields min <= max).  The inserted bits are the reference's for every defined box.
 * Two stated divergences:
 *   - Undefined inputs: glm::ivec3(float) is undefined behaviour for NaN, +-Inf and magnitudes >= 2^31.  Here an entity with such a centre or
 *     extent component is neither inserted nor visible (the reference's result depends on its compiler and CPU).
 *   - Negative extents (a caller's box with min > max by two units or more): TNode::Contains is then an overlap test, where the element rests
 *     depends on the other elements, and the walk may prune a node the frustum misses while the element's own box is in view.  Here such an
 *     entity is visible by the rule above: a superset of the walk's answer, independent of the other entities. */
#define SAILOR_TRACE_FLAT_FLOAT_BOXES 0u  /* what sailor_hip_ecs_sweep does today */
#define SAILOR_TRACE_OCTREE_INT_BOXES 1u  /* RHISceneView::TraceScene as the reference runs it */
#define SAILOR_OCTREE_ROOT_SIZE 264576u   /* RHI/SceneView.h:91-92, 16536 * 16 */
typedef struct SailorSceneTrace {
    uint32_t mode;       /* one of the above; anything else is SAILOR_HIP_ERR_INVALID_ARGUMENT */
    uint32_t rootSize;   /* 0 = SAILOR_OCTREE_ROOT_SIZE; otherwise 2 .. 2^30 (tests use small roots) */
    uint64_t* dInserted; /* device out, ceil(n / 64) words, or NULL: bit i = entity i is in the octree at all (Octree.h:397-437 Insert succeeded);
                            octree mode only (non-NULL in flat mode is SAILOR_HIP_ERR_INVALID_ARGUMENT) */
} SailorSceneTrace;
/* sailor_hip_ecs_sweep_range with a choice of visibility test (trace NULL = flat, exactly sailor_hip_ecs_sweep_range).  World matrices and boxes are
 * the same in both modes.  Only the slice's bits of dVisibility and of trace->dInserted are written; a proper slice of a hierarchy deeper than four
 * levels is refused as there.  Records on the context's stream only: no synchronisation, no host reads. */
SAILOR_HIP_API int sailor_hip_ecs_sweep_traced(SailorHipContext* ctx, uint32_t numEntities,
                                               const SailorTransform* dTransforms, const uint32_t* dParent,
                                               const uint32_t* levelOffsets, uint32_t numLevels,
                                               const SailorAABB* dLocalAabb, const float* planes,
                                               float* dWorld, SailorAABB* dWorldAabb, uint64_t* dVisibility,
                                               uint32_t entityBegin, uint32_t entityEnd, const SailorSceneTrace* trace);
SAILOR_HIP_API int sailor_hip_ecs_range_for_rank(uint32_t numEntities, int32_t rank, int32_t worldSize, uint32_t* outBegin, uint32_t* outEnd,
                                                 uint32_t* outWordsPerRank /* or NULL */);
SAILOR_HIP_API int sailor_hip_exchange_visibility(SailorHipContext* ctx, void* comm, int32_t rank, int32_t worldSize, uint32_t numEntities,
                                                  uint64_t* dVisibility, size_t visibilityWords);

#define SAILOR_RASTER_CLEAR 1u
#define SAILOR_RASTER_CULL_BACK 2u
/* Replaces: the caster draws of one shadow pass, FrameGraph/ShadowPrepassNode.cpp:219-262 with Content/Shaders/ShadowCaster.shader:46-59 (vertex stage:
 * gl_Position = lightMatrix * instance.model * vec4(inPosition, 1)) -- depth only; the rasterisation rules are those of the oracle (1/256-pixel
 * snapping, top-left rule, unfused fp32 depth interpolation, reversed Z: GREATER against a buffer cleared to 0, viewport (0, H, W, -H)).
 *   lightMatrix  : host, mat4 (the pass' push constant, RHIUpdateShadowMapCommand::m_lightMatrix)
 *   dPositions   : device, vec3 per vertex (VertexP3N3T3B3UV2C4::m_position); dIndices: device, 3 x numTriangles
 *   dModels      : device, mat4 per instance (PerInstanceData.model); dInstanceIds: device, numDrawn instance indices, or NULL for 0 .. numDrawn-1
 *   dDepth       : device in/out, width x height floats
 *   flags        : SAILOR_RASTER_CLEAR clears dDepth (and the coarse depth) to 0 first -- a dependent pass (:250-261) draws on top without it;
 *                  SAILOR_RASTER_CULL_BACK discards back faces as the reference's materials do (ECullMode::Back, frontFace counter-clockwise)
 *   dCoarseDepth : device scratch or NULL, sailor_hip_raster_coarse_words(width, height) words belonging to dDepth (cleared with it): lower bounds of the
 *                  depths stored in each 8 x 8 block and each 64 x 64 superblock, used to skip what cannot win any more -- whole triangles, blocks, and
 *                  (round 6, draws of >= 4 096 instances) whole INSTANCES: the box of the mesh's referenced vertices through the instance's matrix -- and,
 *                  behind those, the box itself (8 words) and a queue of "giant" triangles (4 + 24 words per entry, two entries per superblock): a
 *                  triangle that is visible and large on the map is drawn by sixty-four waves of a second kernel instead of block by block by the wave
 *                  that set it up, and a draw of many instances goes out in up to six launches of growing size so that a launch's giants are on the map
 *                  before the next launch starts (a caller that sorts its instances front to back gets most of the later ones skipped).  All of it is
 *                  bounds and scheduling only: the depth buffer is bit for bit the same with and without the workspace, in any drawing order. */
SAILOR_HIP_API size_t sailor_hip_raster_coarse_words(int32_t width, int32_t height);
SAILOR_HIP_API int sailor_hip_raster_depth(SailorHipContext* ctx, const float* lightMatrix, const float* dPositions, const uint32_t* dIndices,
                                           uint32_t numTriangles, const float* dModels, const uint32_t* dInstanceIds, uint32_t numDrawn,
                                           int32_t width, int32_t height, float* dDepth, uint32_t flags, uint32_t* dCoarseDepth);
/* Replaces: the draws of the depth prepass, FrameGraph/DepthPrepassNode.cpp:283-297 with Content/Shaders/DepthOnly.shader:51
 * (gl_Position = frame.projection * (frame.view * (model * position))): the same rasteriser, the camera's matrices from the frame UBO; the reversed-Z
 * projection makes it GREATER against the cleared 0 again.  dDepth is the raw depth attachment LinearizeDepth / SAILOR_CULL_RAW_DEPTH consume.
 * Triangles that cross the near plane (z_clip > w_clip, which includes vertices behind the eye) are cut against it in clip space, as in the oracle. */
SAILOR_HIP_API int sailor_hip_raster_depth_camera(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* dPositions, const uint32_t* dIndices,
                                                  uint32_t numTriangles, const float* dModels, const uint32_t* dInstanceIds, uint32_t numDrawn,
                                                  int32_t width, int32_t height, float* dDepth, uint32_t flags, uint32_t* dCoarseDepth);
/* The fragment stage of ShadowCaster.shader:66-78 on the winning depth of every texel: EVSM moments (format RGBA32F: exp(40 z), its square,
 * -exp(-40 z), its square), or the depth itself (R16F / R32F); texels nothing was drawn to keep the cleared colour 0. */
SAILOR_HIP_API int sailor_hip_shadow_resolve(SailorHipContext* ctx, const float* dDepth, int32_t width, int32_t height, int32_t format, void* dShadowMap);

/* The cascade mesh lists of LightingECS::PrepareCSMPasses (ECS/LightingECS.cpp:287-296: `cascade.m_meshList = sceneView->TraceScene(frustums[k], true)`)
 * as bitmasks over the entities of sailor_hip_ecs_sweep: bit i of mask k = dWorldAabb[i] overlaps the frustum of cascade k (Math/Bounds.cpp:245-260).
 *   cascadePlanes : host, numCascades x 6 x vec4 from sailor_host_extract_frustum_planes_matrix(lightCascadesMatrices[k] * lightMatrix) (:287-292)
 *   dMasks        : device out, numCascades x ceil(numEntities / 64) words, LSB first
 * The removal of meshes already drawn by an earlier cascade of the same kind (:310-327) and the change tracking (:334-366, CSMLightState::Equals :14-38)
 * stay on the host, on these sets. */
SAILOR_HIP_API int sailor_hip_csm_caster_masks(SailorHipContext* ctx, uint32_t numEntities, const SailorAABB* dWorldAabb, const float* cascadePlanes,
                                               uint32_t numCascades, uint64_t* dMasks);
/* The same lists as LightingECS.cpp:296 really builds them, `TraceScene(frustums[k], true)` through the octree: trace as for sailor_hip_ecs_sweep_traced
 * (NULL = flat, exactly sailor_hip_csm_caster_masks); the root's box is tested against each cascade's frustum.  trace->dInserted, when given, gets
 * ceil(numEntities / 64) words, the same for every cascade.  Records only. */
SAILOR_HIP_API int sailor_hip_csm_caster_masks_traced(SailorHipContext* ctx, uint32_t numEntities, const SailorAABB* dWorldAabb, const float* cascadePlanes,
                                                      uint32_t numCascades, uint64_t* dMasks, const SailorSceneTrace* trace);

/* Replaces: the host loop that fills a shadow pass's per-instance SSBO, FrameGraph/ShadowPrepassNode.cpp:155-201 (a memcpy of every proxy's
 * `gpuMatricesData` run into the `data` binding: ShadowPrepassNode::PerInstanceData { mat4 model; }, 64 bytes) -- from a cascade's bitmask, on the device.
 * One job: for every set bit i of dMask in [begin, end), in ASCENDING i, out[j] = dInstances[i].model; *dCount = the number of set bits in the range.
 *   dMask    : device, bit i = instance i of the scene's SSBO, LSB first (the layout of sailor_hip_csm_caster_masks / sailor_host_csm_plan_passes);
 *              only words that hold bits of [begin, end) are read, bits at or past `end` are ignored
 *   dOut     : device, capacity x 16 floats, 16-byte aligned; with capacity < count only the first `capacity` matrices are written, and nothing behind them
 *   dCount   : device, one word, always the full count
 * The order inside a batch is the canonical one (by index); the reference's is its octree's walk order, and the rasteriser's result does not depend on it.
 * The output is a pure function of the inputs.  Records on the context's stream only: no upload, no read-back, no synchronisation (the jobs travel in the
 * kernels' arguments).  dWorkspace: device scratch, 4-byte aligned, sailor_hip_shadow_gather_workspace_bytes(jobs, numJobs) bytes -- 4 per 1 024 bits of
 * every job's range; it depends on the ranges only. */
typedef struct SailorShadowGatherJob {
    const uint64_t* dMask;
    uint32_t begin, end;
    float* dOut;
    uint32_t capacity;
    uint32_t _pad;
    uint32_t* dCount;
} SailorShadowGatherJob;
SAILOR_HIP_API size_t sailor_hip_shadow_gather_workspace_bytes(const SailorShadowGatherJob* jobs, uint32_t numJobs);
/* numJobs jobs (passes x batches) over one instance buffer in one call: two launches per 32 jobs.  The jobs' outputs must not overlap. */
SAILOR_HIP_API int sailor_hip_shadow_gather_instances_batched(SailorHipContext* ctx, const SailorPerInstanceData* dInstances, uint32_t numInstances,
                                                              const SailorShadowGatherJob* jobs, uint32_t numJobs, void* dWorkspace, size_t workspaceBytes);
SAILOR_HIP_API int sailor_hip_shadow_gather_instances(SailorHipContext* ctx, const SailorPerInstanceData* dInstances, uint32_t numInstances,
                                                      const uint64_t* dMask, uint32_t begin, uint32_t end, float* dOut, uint32_t capacity, uint32_t* dCount,
                                                      void* dWorkspace, size_t workspaceBytes);

/* Replaces: FrustumCulling of Content/Shaders/ComputeMeshCulling.shader:96-110 (+ CreateViewFrustum, Math.glsl:185-222)
 * for the Dispatch at RHI/Batch.hpp:188; writes PerInstanceData::isCulled in place for the instances
 * [firstInstanceIndex, firstInstanceIndex + numInstances).  Hi-Z occlusion (the shader's OCCLUSION_CULLING define) is out of
 * scope. */
SAILOR_HIP_API int sailor_hip_mesh_frustum_cull(SailorHipContext* ctx, const SailorUboFrameData* frame,
                                                SailorPerInstanceData* dInstances, uint32_t numInstances, uint32_t firstInstanceIndex);

/* Replaces: the whole main() of Content/Shaders/ComputeMeshCulling.shader:119-177 built without OCCLUSION_CULLING, for the same
 * Dispatch (RHI/Batch.hpp:177-188; push constants numBatches / numInstances / firstInstanceIndex):
 *   step 2 (:126-144)  isCulled over the instance window, as sailor_hip_mesh_frustum_cull;
 *   step 3 (:146-177)  per indirect draw a stable in-place compaction of its instance records
 *                      [firstInstance, firstInstance + instanceCount) by isCulled == 0, and instanceCount = number kept.
 * Every flag is written before any batch is compacted (the canonical reading of the shader's cross-workgroup race).  The batches
 * own disjoint instance ranges inside the buffer and their instanceCounts add up to at most numInstances (exactly numInstances at
 * RHI/Batch.hpp:158-159,183).  Records behind a batch's kept prefix keep their old contents, as in the shader.
 *   dBatches   : device in/out, numBatches x SailorDrawIndexedIndirectData ("drawIndexedIndirect", set 2 binding 0)
 *   dWorkspace : device scratch, 256-byte aligned, sailor_hip_mesh_cull_workspace_bytes(numInstances, numBatches) bytes */
/* The Hi-Z pyramid ("depthHighZ", set 0 binding 0 of ComputeMeshCulling.shader; render target DepthHighZ of Content/DefaultRenderer.renderer:51-57:
 * R32_SFLOAT, mips, sampler reduction Min): level-major, level l = max(height >> l, 1) rows of max(width >> l, 1) floats of raw reversed-Z depth. */
typedef struct SailorHiZDesc {
    const float* pyramid;
    int32_t width, height, levels;
} SailorHiZDesc;

/* Replaces: Content/Shaders/ComputeDepthHighZ.shader:22-30 for one Dispatch of FrameGraph/DepthHighZNode.cpp:90-95 -- out(pos) = the minimum
 * over the bilinear footprint of the source at (pos + 0.5) / outputSize (texels with non-zero weight, clamp-to-edge: x = u W - 0.5, i0 = floor(x),
 * i1 = i0 + 1 on the floor itself, never floor(x + 1.0f), which rounds up to the next integer for x = -2^-25).
 * One stated divergence (the sampler convention): a neighbour texel counts whenever the FP32 fraction of x is not exactly 0.  For a same-size step
 * the exact position ((2 i + 1) src - dst) / (2 dst) is an integer, but the fp32 evaluation leaves a non-zero fraction on 25 of the 960 columns
 * of a 960 -> 960 step (the shipped pyramid's own first step in x) and on 2 of the 131 columns of 131 -> 131; those texels take the minimum with
 * the next column as well.  Any hardware sampler quantises such a fraction to 0.  The effect is conservative (a farther depth).  None for powers of
 * two, 48 -> 16, 36 -> 12, 96 -> 96 and every 2:1 step.  Counted by tests/test_mesh_cull_cpu.py against exact rational sample positions. */
SAILOR_HIP_API int sailor_hip_hiz_downscale(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst,
                                            int32_t dstWidth, int32_t dstHeight);
/* The node's whole loop (DepthHighZNode.cpp:78-96): mip 0 from the depth attachment "src", mip i + 1 from mip i. */
SAILOR_HIP_API int sailor_hip_hiz_build(SailorHipContext* ctx, const float* dDepth, int32_t depthWidth, int32_t depthHeight, float* dPyramid,
                                        int32_t width, int32_t height, int32_t levels);
/* sailor_hip_mesh_frustum_cull with the shader's OCCLUSION_CULLING define when `hiz` is given: isCulled = FrustumCulling || OcclusionCulling
 * (ComputeMeshCulling.shader:62-94,136-140; ProjectSphere Math.glsl:296-315; floor(log2()) of the mip selection taken from the exponent field). */
SAILOR_HIP_API int sailor_hip_mesh_cull_flags(SailorHipContext* ctx, const SailorUboFrameData* frame, SailorPerInstanceData* dInstances,
                                              uint32_t numInstances, uint32_t firstInstanceIndex, const SailorHiZDesc* hiz);
SAILOR_HIP_API size_t sailor_hip_mesh_cull_workspace_bytes(uint32_t numInstances, uint32_t numBatches);
/* sailor_hip_mesh_cull_compact (below) with the Hi-Z pyramid: the shader as shipped (`defines: - OCCLUSION_CULLING`); hiz == NULL = frustum only */
SAILOR_HIP_API int sailor_hip_mesh_cull_compact_ex(SailorHipContext* ctx, const SailorUboFrameData* frame, SailorPerInstanceData* dInstances,
                                                   uint32_t numInstances, uint32_t firstInstanceIndex, SailorDrawIndexedIndirectData* dBatches,
                                                   uint32_t numBatches, void* dWorkspace, size_t workspaceBytes, const SailorHiZDesc* hiz);
SAILOR_HIP_API int sailor_hip_mesh_cull_compact(SailorHipContext* ctx, const SailorUboFrameData* frame, SailorPerInstanceData* dInstances,
                                                uint32_t numInstances, uint32_t firstInstanceIndex, SailorDrawIndexedIndirectData* dBatches,
                                                uint32_t numBatches, void* dWorkspace, size_t workspaceBytes);

/* ---- EyeAdaptation: histogram, average luminance, tone map -- the node right behind the two RenderScene passes ----------------
 * Replaces: the two Dispatches and the full-screen draw recorded by EyeAdaptationNode::Process (FrameGraph/EyeAdaptationNode.cpp:22-221):
 * Content/Shaders/ComputeHistogram.shader, Content/Shaders/ComputeAverageLuminance.shader and Content/Shaders/Tonemapping.shader with
 * Content/Shaders/Formats.glsl:1-51.  Targets are fp32 (the project's canonical form of R16G16B16A16_SFLOAT / R16_SFLOAT,
 * FrameGraphParser.cpp:196): float4 radiance in -- what sailor_hip_shade* writes --, float4 out, one fp32 word of adapted luminance.
 * log2 / exp2 are fixed fp32 algorithms (sailor_amd/csrc/eye_adaptation.hip: canonical_log2f, canonical_exp2f), restated in
 * tests/eye_adaptation_ref.py; counts, luminance and image are reproducible bit for bit.
 * Kept from the reference: the histogram counts only x < 16 * (width / 16), y < 16 * (height / 16) (its dispatch is extent / 16 by integer
 * division, :173-174) while numPixels is width * height; the weighted sum is uint32 and wraps at 8K; a black pixel under LUMINANCE is NaN
 * (Formats.glsl:18 divides by X + Y + Z).  Defined where GLSL is not: a NaN luminance counts in bin 0, +inf in bin 255. */

/* the push constants of the two Dispatches (EyeAdaptationNode.cpp:154-170; ComputeHistogram.shader:21-25, ComputeAverageLuminance.shader:21-27) */
typedef struct SailorEyeAdaptationConstants {
    float minLog2Luminance;      /* -8 */
    float invLog2LuminanceRange; /* 1 / 12 */
    float log2LuminanceRange;    /* 12 */
    float numPixels;             /* (float)width * height */
    float timeCoeff;             /* clamp(1 - exp2(-deltaTime * 3.6), 0, 1) */
} SailorEyeAdaptationConstants;

/* Tonemapping.shader:6-9 defines; ACES wins over UNCHARTED2 (#if / #elif, :150-154) */
#define SAILOR_TONEMAP_ACES 1u
#define SAILOR_TONEMAP_UNCHARTED2 2u
#define SAILOR_TONEMAP_LUMINANCE 4u

/* The node's state: caller-owned device memory of sailor_hip_eye_adaptation_state_size() bytes, 16-byte aligned -- the `histogram` SSBO
 * (256 uint32 counts, EyeAdaptationNode.cpp:68) and m_averageLuminance (:87-97).  reset zeroes the counts and stores the luminance (the
 * reference clears it to 0.5, :97).  state_views: the counts and the luminance word inside it (either out pointer may be NULL) -- for tests,
 * and for a caller that sums the band histograms of a split frame itself (sailor_hip_allgather_u32). */
SAILOR_HIP_API size_t sailor_hip_eye_adaptation_state_size(void);
SAILOR_HIP_API int sailor_hip_eye_adaptation_reset(SailorHipContext* ctx, void* dState, float initialLuminance);
SAILOR_HIP_API int sailor_hip_eye_adaptation_state_views(const void* dState, const uint32_t** outCounts, const float** outLuminance);
/* Replaces: the Dispatch at EyeAdaptationNode.cpp:173-176 = ComputeHistogram.shader:37-83.  ADDS the band's counts to the state's.
 *   dColor : device, float4 per pixel, the rows of `band` (first row = band->fbRowBegin), 16-byte aligned */
SAILOR_HIP_API int sailor_hip_luminance_histogram(SailorHipContext* ctx, const float* dColor, int32_t width, int32_t height, const SailorBand* band,
                                                  const SailorEyeAdaptationConstants* constants, void* dState);
/* Replaces: the Dispatch at EyeAdaptationNode.cpp:179-182 = ComputeAverageLuminance.shader:39-78: reduces the counts, zeroes them for the
 * next frame and moves the luminance towards the frame's average by timeCoeff. */
SAILOR_HIP_API int sailor_hip_average_luminance(SailorHipContext* ctx, const SailorEyeAdaptationConstants* constants, void* dState);
/* Replaces: the render pass and DrawIndexed(6) at EyeAdaptationNode.cpp:192-218 = Tonemapping.shader:135-161.  The draw samples a source of
 * the target's size at texel centres: a texel fetch, so one width / height serves both.
 *   dColor / dOut : device, float4 per pixel, the rows of `band`; operatorFlags: SAILOR_TONEMAP_* (anything else is refused)
 *   whitePoint4, exposure : data.whitePoint / data.exposure.x (:52-56; the shipped node: (1.4, 1.5, 1.4), 1) */
SAILOR_HIP_API int sailor_hip_tonemap(SailorHipContext* ctx, const float* dColor, float* dOut, int32_t width, int32_t height, const SailorBand* band,
                                      uint32_t operatorFlags, const float* whitePoint4, float exposure, const void* dState);
/* The node's whole sequence on the whole frame: histogram, average, tone map (EyeAdaptationNode.cpp:173-218). */
SAILOR_HIP_API int sailor_hip_eye_adaptation(SailorHipContext* ctx, const float* dColor, float* dOut, int32_t width, int32_t height,
                                             const SailorEyeAdaptationConstants* constants, uint32_t operatorFlags, const float* whitePoint4,
                                             float exposure, void* dState);

/* ---- HBAO: the producer of g_AO (Standard.shader:386 reads it through g_aoSampler) ------------------------------------------------------
 * Replaces: the GPU work of the HBAO block of the shipped frame graph (DefaultRenderer.renderer:202-264): the Blit DepthBuffer -> HalfDepth
 * (FrameGraph/BlitNode.cpp:21-124), the PostProcess draw (FrameGraph/PostProcessNode.cpp:22-202) with Content/Shaders/HBAO.shader:81-249 and the
 * two PostProcess draws with Content/Shaders/HBAO_Blur.shader:67-111 (VERTICAL, HORIZONTAL).  (DepthHighZ between them: sailor_hip_hiz_*.)
 * Every image is a single-channel fp32 plane in device memory, row 0 = top, texel (i, j) of a w x h target has fragTexcoord
 * ((i + 0.5) / w, (j + 0.5) / h); the extents of a call are independent of one another.  The R8_UNORM targets (AO, TemporaryR8, g_AO) are fp32
 * planes that hold what texture() would return from the 8-bit target: rintf(min(max(v, 0), 1) * 255) / 255, NaN -> 0.
 * The shaders are evaluated as written, in their order, one IEEE rounding per operation, with the evaluation order fixed above for the tone map:
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, mat4 * vec4 row by row left to right, v / s = one division per component, length = sqrt(dot),
 * normalize(v) = v / length(v), rcp(x) = 1 / x, mix(a, b, t) = a (1 - t) + b t, products left to right; tests/hbao_ref.py restates them and the
 * results are reproducible bit for bit.  Decisions (HBAO.shader lines):
 *   - main() normalises the normal twice (:116, :199): both kept;  ClipSpaceToViewSpace gets (uv.x, uv.y, depth, 1), not NDC (:91, :112-114): literal;
 *   - depthSampler / aoSampler: bilinear, clamp-to-edge, the taps and weights of sailor_amd/csrc/sampling.h evaluated per fetch (no corner plane);
 *   - noiseSampler: nearest, repeat: texel floor(u * nw) mod nw;  round() in SnapTexel: half to even;
 *   - screenSpace1Meter (:211) is NaN for every perspective projection (clip w of (0, 1, 0, 1) is 0, x / w = 0 / 0), so sampleRadius = occlusionRadius (:213);
 *   - sinS = sin(PI / 2 - acos(x)) (:133) is evaluated as x, without a clamp;  saturate(x) = x < 0 ? 0 : (x > 1 ? 1 : x) passes a NaN on;
 *   - non-finite sample coordinates (depth 0, inf, NaN) take the saturating float -> int conversion with NaN -> 0 in the tap computation;
 *   - the sky check (:190-194) and screenSpaceRadius < 1 (:225) store 1; distanceFactor (:138) is not clamped;
 *   - the blur's exp2 is the fixed fp32 algorithm of sailor_amd/csrc/canonical_math.h; its loops run over float i = 1 .. radius, all + taps first. */

/* HBAO.shader:50-57 PostProcessDataUBO (std140: floats at 0, 4, 8, 12, 16) */
typedef struct SailorHbaoParams {
    float occlusionRadius;      /* shipped: 700 */
    float occlusionPower;       /* 1.5 */
    float occlusionAttenuation; /* 0.1 */
    float occlusionBias;        /* 0.05 */
    float noiseScale;           /* 25 */
} SailorHbaoParams;

/* HBAO_Blur.shader:54-59 PostProcessDataUBO (floats at 0, 4, 8) */
typedef struct SailorHbaoBlurParams {
    float sharpness;     /* shipped: 0.5 */
    float distanceScale; /* 2 */
    float radius;        /* 5; at most 64 */
} SailorHbaoBlurParams;

/* Replaces: the vkCmdBlitImage with VK_FILTER_NEAREST of a scaled single-channel image (BlitNode.cpp:88-96: depth formats are blitted with Nearest).
 * Destination texel (i, j) takes source texel (((2 i + 1) * srcWidth) / (2 * dstWidth), ((2 j + 1) * srcHeight) / (2 * dstHeight)), integer division:
 * the texel that contains the destination centre.  (Equal extents: sailor_hip_buffer_copy.) */
SAILOR_HIP_API int sailor_hip_blit_nearest(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight,
                                           float* dDst, int32_t dstWidth, int32_t dstHeight);
/* Replaces: the DrawIndexed(6) of PostProcessNode::Process (PostProcessNode.cpp:176-199) with Content/Shaders/HBAO.shader:185-249.
 *   frame  : invProjection, cameraZNearZFar.x and viewportSize.y are read
 *   dDepth : `depthSampler` (HalfDepth in the shipped file);  dNoise : `noiseSampler`, noiseWidth x noiseHeight decoded linear float4 texels, 16-byte aligned
 *   dAo    : device out, the `color` target */
SAILOR_HIP_API int sailor_hip_hbao(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* dDepth, int32_t depthWidth, int32_t depthHeight,
                                   const float* dNoise, int32_t noiseWidth, int32_t noiseHeight, const SailorHbaoParams* params,
                                   float* dAo, int32_t width, int32_t height);
/* Replaces: the same draw with Content/Shaders/HBAO_Blur.shader:82-111; vertical != 0 is the VERTICAL define (aoPixelSize.x = 0, :88-89), 0 HORIZONTAL.
 *   dAo : `aoSampler`;  dDepth : `depthSampler` (the raw full-resolution DepthBuffer in the shipped file);  dDst : device out, the `color` target */
SAILOR_HIP_API int sailor_hip_hbao_blur_pass(SailorHipContext* ctx, const float* dAo, int32_t aoWidth, int32_t aoHeight,
                                             const float* dDepth, int32_t depthWidth, int32_t depthHeight, const SailorHbaoBlurParams* params,
                                             float* dDst, int32_t width, int32_t height, int32_t vertical);
/* The block's four launches (DefaultRenderer.renderer:204-264 without DepthHighZ): blit dDepth -> dHalfDepth, HBAO on dHalfDepth -> dAo, vertical
 * blur of dAo against dDepth -> dTemp, horizontal blur of dTemp against dDepth -> dOut (g_AO).  The intermediates are the caller's; the launches are
 * those of the four single calls.  Every argument is checked before the first launch. */
SAILOR_HIP_API int sailor_hip_hbao_chain(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* dDepth, int32_t depthWidth, int32_t depthHeight,
                                         float* dHalfDepth, int32_t halfWidth, int32_t halfHeight, const float* dNoise, int32_t noiseWidth, int32_t noiseHeight,
                                         const SailorHbaoParams* params, float* dAo, int32_t aoWidth, int32_t aoHeight,
                                         const SailorHbaoBlurParams* blurParams, float* dTemp, int32_t tempWidth, int32_t tempHeight,
                                         float* dOut, int32_t outWidth, int32_t outHeight);

/* ---- The frame's tail: motion blur into Main and the Debug view into BackBuffer (DefaultRenderer.renderer:322-353) -----------------------
 * Replaces: the GPU work of the last two PostProcess draws (FrameGraph/PostProcessNode.cpp:176-199) of the shipped frame graph, with
 * Content/Shaders/MotionBlur.shader:63-102 and Content/Shaders/Debug.shader:115-178.  Colour images are RGBA32F device planes, 16-byte aligned; depth,
 * linear depth and g_AO are single-channel fp32 planes; row 0 = top; texel (i, j) of a w x h target has fragTexcoord ((i + 0.5) / w, (j + 0.5) / h) and
 * gl_FragCoord (i + 0.5, j + 0.5); the extents of a call are independent of one another.  The shaders are evaluated as written, one IEEE rounding
 * per written operation, with the evaluation orders fixed above for HBAO (mat4 * vec4 row by row left to right, v / s = one division per component,
 * length = sqrt(dot), mix(a, b, t) = a (1 - t) + b t); tests/tail_ref.py restates them and the results are reproducible bit for bit.  The entry
 * points only record: no synchronisation, capturable into a graph.  Decisions:
 *   - inverse(frame.projection), inverse(frame.view) and previousFrame.projection * previousFrame.view are uniform per draw: computed once on the host
 *     with the glm order of sailor_host_mat4_inverse / sailor_host_mat4_mul and passed to the kernel by value.  frame.invProjection is not used: the
 *     shader writes the literal inverse(frame.projection) (MotionBlur.shader:69);
 *   - min(x, y) = y < x ? y : x and max(x, y) = x < y ? y : x, the GLSL definitions: min(1, NaN) = 1.  On the first frame the previous frame data
 *     is all zeros (RHIFrameGraph.cpp:189), previousClipPos is 0 / 0 everywhere and the velocity is (intensity, intensity);
 *   - the velocity has no lower clamp (:81-82); clamp(x, 0, 1) = min(max(x, 0), 1); length = sqrt(dot) and the early-out `<= 0.0001` as written (:87);
 *   - int(data.samples) truncates, the loop runs int(samples) - 1 taps, the division is by float(data.samples); output alpha is 1;
 *   - depthSampler / colorSampler / ldrSceneSampler / g_aoSampler: bilinear, clamp-to-edge, the taps and weights of sailor_amd/csrc/sampling.h
 *     evaluated per fetch, non-finite coordinates through the saturating float -> int conversion (NaN -> 0) that HBAO documents;
 *     linearDepthSampler: Nearest (DefaultRenderer.renderer:85-90), texel min(max(int(floor(u * w)), 0), w - 1);
 *   - LIGHT_TILES adds 0.05 once per listed light, as sequential fp32 additions onto linearDepth / 50000 (not n * 0.05). */

/* MotionBlur.shader:50-55 PostProcessDataUBO (std140: floats at 0, 4, 8) */
typedef struct SailorMotionBlurParams {
    float intensity; /* shipped: 1 (DefaultRenderer.renderer:328-330) */
    float samples;   /* 10; finite, within [1, 64] */
    float maxSpeed;  /* 50; not 0 */
} SailorMotionBlurParams;

/* Debug.shader's define sets that have an entry point: none, or exactly one of AO, LIGHT_TILES, CASCADES (:119, :121, :145) */
#define SAILOR_DEBUG_VIEW_SCENE 0
#define SAILOR_DEBUG_VIEW_AO 1
#define SAILOR_DEBUG_VIEW_LIGHT_TILES 2
#define SAILOR_DEBUG_VIEW_CASCADES 3

/* Replaces: the DrawIndexed(6) of PostProcessNode::Process with Content/Shaders/MotionBlur.shader:63-102.
 *   frame / previousFrame : `frameData` / `previousFrameData` (set 0, bindings 0 and 1); projection and view of both are read
 *   dDepth : `depthSampler` (the raw DepthBuffer);  dColor : `colorSampler` (Secondary);  dOut : device out, the `color` target (Main, level 0)
 * Refused with SAILOR_HIP_ERR_INVALID_ARGUMENT, recording nothing: a null or misaligned pointer, a non-positive extent, samples not finite, below 1 or
 * above 64, maxSpeed == 0, dOut overlapping dColor. */
SAILOR_HIP_API int sailor_hip_motion_blur(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorUboFrameData* previousFrame,
                                          const float* dDepth, int32_t depthWidth, int32_t depthHeight, const float* dColor, int32_t colorWidth, int32_t colorHeight,
                                          const SailorMotionBlurParams* params, float* dOut, int32_t width, int32_t height);
/* Replaces: the same draw with Content/Shaders/Debug.shader:115-178 under the define set `mode` names.
 *   frame        : viewportSize (LIGHT_TILES) and cameraZNearZFar.y (CASCADES) are read
 *   dLdrScene    : `ldrSceneSampler` (SCENE, CASCADES);  dLinearDepth : `linearDepthSampler` (LIGHT_TILES, CASCADES)
 *   dLightsGrid / dCulledLights : the light cull's two SSBOs (LIGHT_TILES; ignored otherwise);  dAo : `g_aoSampler` (AO)
 *   dOut         : device out, the `color` target (BackBuffer)
 * A mode that needs a buffer it was given as null is refused with SAILOR_HIP_ERR_INVALID_ARGUMENT, like a misaligned pointer, a non-positive extent, an
 * unknown mode, dOut overlapping dLdrScene, and -- LIGHT_TILES -- a target whose extent is not frame.viewportSize (gl_FragCoord indexes the frame's tiles).
 * A list entry past the reference's culledLights capacity (tiles * 128 + 1 words) ends its list like the sentinel. */
SAILOR_HIP_API int sailor_hip_debug_view(SailorHipContext* ctx, const SailorUboFrameData* frame, int32_t mode, const float* dLdrScene, int32_t sceneWidth,
                                         int32_t sceneHeight, const float* dLinearDepth, int32_t depthWidth, int32_t depthHeight,
                                         const SailorLightsGrid* dLightsGrid, const uint32_t* dCulledLights, const float* dAo, int32_t aoWidth, int32_t aoHeight,
                                         float* dOut, int32_t width, int32_t height);

/* ---- Post effects: Blur.shader without EVSM, ChromaticAberation.shader, the scaled Linear blit ------------------------------------------------
 * Replaces: the GPU work of the PostProcess and Blit entries the shipped frame graph names in its commented entries (DefaultRenderer.renderer:157-181,
 * :355-366) and of a blur chain over its unused QuarterMain1 / QuarterMain2 targets: the DrawIndexed(6) of PostProcessNode::Process
 * (FrameGraph/PostProcessNode.cpp:176-199) with Content/Shaders/Blur.shader:66-98 or Content/Shaders/ChromaticAberation.shader:62-73, and the
 * vkCmdBlitImage with VK_FILTER_LINEAR of BlitNode::Process (FrameGraph/BlitNode.cpp:88-96).  Images are fp32 RGBA planes in device memory, 16-byte
 * aligned (the blit also takes one-channel planes); row 0 = top; texel (i, j) of a w x h target has fragTexcoord ((i + 0.5) / w, (j + 0.5) / h); source
 * and target extents are independent.  The shaders are evaluated as written, left to right, one IEEE rounding per written operation; every texture() is
 * bilinear, clamp-to-edge, the taps and weights of sailor_amd/csrc/sampling.h evaluated per fetch; tests/effects_ref.py restates the four passes in
 * NumPy float32 and the results are reproducible bit for bit.  The entry points only record: no synchronisation, capturable into a graph.  Decisions:
 *   - texelSize = 1.0f / textureSize(colorSampler, 0) (Blur.shader:68) is uniform per draw: (1.0f / srcWidth, 1.0f / srcHeight), computed once on the
 *     host.  VERTICAL zeroes x (:70-72), HORIZONTAL zeroes y (:74-76); neither blurs along the diagonal, both put every tap at uv: all four are legal;
 *   - Gauss (no RADIAL, no EVSM; GaussianBlur, Lighting.glsl:129-159): radius = uint(data.blurRadius.x) truncates, blurRadius = min(radius, 12), the
 *     loop runs i = 0 .. blurRadius - 1 with off = float(i) * texelSize, color = texture(uv + off) + texture(uv - off), pixelSum = pixelSum + color *
 *     weights[blurRadius - 1][i].  Tap 0 reads the centre twice: kept.  blurRadius == 0 writes rgb 0;
 *   - the shader assigns only outColor.xyz (:94), so the reference's alpha is undefined: THIS PATH WRITES ALPHA 0.0f;
 *   - RADIAL (:78-89) wins over EVSM by the shader's #ifdef order: direction = ((blurCenter.xy - uv) * texelSize) * blurRadius.x, the loop is
 *     for (index = 0; float(index) < blurSampleCount.x; ++index) { sum += texture(uv); uv += direction; }, the result sum / blurSampleCount.x, one
 *     division per component, all four channels: a fractional count runs ceil(count) taps and divides by the fraction.  The reference has no cap on the
 *     count; this path refuses more than 256, like the motion blur's 64;
 *   - the radial taps' coordinates are driven by parameters and may leave the int range: they take the saturating float -> int conversion (NaN -> 0)
 *     that HBAO documents, as do the Gauss and aberration taps.  The blit's coordinates are always finite and take the plain conversion;
 *   - chromatic aberration: x = abs(u - 0.5f) / 0.5f, pow(x, 4) = (x * x) * (x * x) (products, as the sky's small integer powers), per channel c
 *     p = offset.c * d and ONE fetch at (u - p, v - p); out = (r of the first, g of the second, b of the third, 1).  The shader's first fetch (:64) is
 *     overwritten at :72 and is not made;
 *   - the Linear blit: destination texel (i, j) = texture() of the source at the texel's own fragTexcoord.  A 2 : 1 blit of power-of-two extents is
 *     the mean of 2 x 2 texels with weights of exactly 0.5, in lerp2's order. */

/* Blur.shader:54-59 PostProcessDataUBO (std140: vec4s at 0, 16, 32) */
typedef struct SailorBlurParams {
    float blurRadius[4];      /* .x is read; the shipped comments: 20 (RADIAL), 4 (HORIZONTAL) (DefaultRenderer.renderer:164, :178) */
    float blurCenter[4];      /* .xy, RADIAL */
    float blurSampleCount[4]; /* .x, RADIAL; finite, within [1, 256] */
} SailorBlurParams;

/* ChromaticAberation.shader:52-55 PostProcessDataUBO */
typedef struct SailorChromaticAberrationParams {
    float offset[4]; /* .xyz; shipped comment: (0.00225, 0.00345, 0.00455) (DefaultRenderer.renderer:362) */
} SailorChromaticAberrationParams;

/* Blur.shader's defines (:7-11) that this entry point reads; EVSM without RADIAL is sailor_hip_evsm_blur_pass */
#define SAILOR_BLUR_HORIZONTAL 1u
#define SAILOR_BLUR_VERTICAL 2u
#define SAILOR_BLUR_RADIAL 4u

/* Replaces: the DrawIndexed(6) of PostProcessNode::Process with Content/Shaders/Blur.shader:66-98 under a define set without EVSM, or with RADIAL.
 *   dSrc : `colorSampler`, srcHeight x srcWidth float4;  dOut : device out, the `color` target, height x width float4
 * Refused with SAILOR_HIP_ERR_INVALID_ARGUMENT, recording nothing and leaving dOut untouched: a null context, params or pointer, a pointer that is not
 * 16-byte aligned, an extent outside 1 .. 32768, dOut overlapping dSrc, unknown flag bits; without RADIAL blurRadius.x not finite, below 0 or >= 2^32
 * (uint() of these is undefined; any value >= 12 caps at 12); with RADIAL blurRadius.x or blurCenter.xy not finite, blurSampleCount.x not finite, below 1
 * or above 256. */
SAILOR_HIP_API int sailor_hip_blur(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, const SailorBlurParams* params,
                                   uint32_t flags, float* dOut, int32_t width, int32_t height);
/* Replaces: the same draw with Content/Shaders/ChromaticAberation.shader:62-73.  Refused like sailor_hip_blur, and for offset.xyz not finite. */
SAILOR_HIP_API int sailor_hip_chromatic_aberration(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight,
                                                   const SailorChromaticAberrationParams* params, float* dOut, int32_t width, int32_t height);
/* Replaces: the vkCmdBlitImage with VK_FILTER_LINEAR of a whole scaled image (BlitNode.cpp:88-96: colour formats are blitted with Linear).
 *   channels : 4 (float4 texels, 16-byte aligned planes) or 1 (float texels, 4-byte aligned); anything else is refused, like a null or misaligned
 *   pointer, an extent outside 1 .. 32768 and dDst overlapping dSrc.  (Equal extents: sailor_hip_buffer_copy; Nearest: sailor_hip_blit_nearest.) */
SAILOR_HIP_API int sailor_hip_blit_linear(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight,
                                          float* dDst, int32_t dstWidth, int32_t dstHeight, int32_t channels);

/* ---- Sky: the producer of the `Sky` target and of g_skyCubemap (EnvironmentNode.cpp bakes g_envCubemap / g_irradianceCubemap from it) ------
 * Replaces: the GPU work of SkyNode::Process (FrameGraph/SkyNode.cpp:524-818) with Content/Shaders/Sky.shader under the define sets {FILL}, {},
 * {SUN} and {COMPOSE}.  Every image is RGBA32F in device memory, 16-byte aligned (the reference: R16G16B16A16_SFLOAT), row 0 = top, texel (i, j)
 * of a w x h target has the quad's inTexcoord ((i + 0.5) / w, (j + 0.5) / h); alpha is stored as 0.  The arithmetic is fixed operation by
 * operation (sailor_amd/csrc/sky.hip's header lists the decisions; tests/sky_ref.py restates it in NumPy float32): every branch is decided by
 * geometry evaluated in fp32 exactly as written, exp is the fixed algorithm of canonical_math.h with its argument clamp, and only the sums over
 * the 127 view steps are reassociated.  These five entry points behave as the reference does with m_cloudsDensity == 0 (SkyNode.cpp:604-609);
 * the clouds, and the star points and sun shafts of the region "Stars & Clouds" (:692-747), have entry points of their own below.
 * All of them record only (no synchronisation, capturable). */

/* Sky.shader:116-136 PostProcessDataUBO == SkyNode::SkyParams (SkyNode.h:48-67), std140: a vec4 at 0, then 4-byte scalars at 16, 20, .. 80.  84 bytes. */
typedef struct SailorSkyParams {
    float lightDirection[4];
    float cloudsAttenuation1;
    float cloudsAttenuation2;
    float cloudsDensity;
    float cloudsCoverage;
    float phaseInfluence1;
    float phaseInfluence2;
    float eccentrisy1;
    float eccentrisy2;
    float fog;
    float sunIntensity;
    float ambient;
    int32_t scatteringSteps;
    float scatteringDensity;
    float scatteringIntensity;
    float scatteringPhase;
    float sunShaftsIntensity;
    int32_t sunShaftsDistance;
} SailorSkyParams;

/* Replaces: the draw "Sky" (SkyNode.cpp:536-563), define FILL = Sky.shader:717-734: SkyLighting with the Earth test of IntersectSphere (:233-243).
 *   frame : view, invProjection and cameraPosition (centimetres) are read;  dSky : device out, height x width float4 (the node: 256 x 256) */
SAILOR_HIP_API int sailor_hip_sky_fill(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params,
                                       float* dSky, int32_t width, int32_t height);
/* Replaces: one face of "Generate Environment Map" (SkyNode.cpp:764-797), no define: the same integral without the Earth test, under the view
 * matrix of `face` and the 90 degree PerspectiveRH(.., 0.1, 1000) of SkyNode.cpp:487-495 (sailor_host_sky_face_matrices).
 *   cameraPosition3 : host, the scene camera's position in centimetres (frameData.m_cameraPosition, :503)
 *   dCube : device in/out, the level-major RGBA32F cube chain of sailor_hip_generate_mipmaps_cube; face `face` of level 0 is written */
SAILOR_HIP_API int sailor_hip_sky_env_face(SailorHipContext* ctx, const float* cameraPosition3, const SailorSkyParams* params,
                                           float* dCube, int32_t size, int32_t face);
/* Replaces: the draw "Sun" (SkyNode.cpp:611-642), define SUN = Sky.shader:693-715 with the SUN branches of SkyLighting (:309-316, :360-374).
 *   dClouds : `cloudsSampler` (:710).  NULL = the cleared m_pCloudsTexture, alpha 0; a plane is SAILOR_HIP_ERR_UNSUPPORTED here: sailor_hip_sky_sun_clouds takes it
 *   dSun    : device out, height x width float4 (the node: 32 x 32) */
SAILOR_HIP_API int sailor_hip_sky_sun(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params,
                                      const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight, float* dSun, int32_t width, int32_t height);
/* Replaces: the draw "Compose" (SkyNode.cpp:644-680), define COMPOSE = Sky.shader:613-643: `skySampler` bilinear with Repeat addressing, `sunSampler`
 * bilinear clamp-to-edge inside the +-SunAngularR window, merged by max(out, mix(out, sun, min(1, dot(sun, sun)))).
 *   dOut : device out, float4 per pixel of the width x height target, the rows of `band` only (first row = band->fbRowBegin) */
SAILOR_HIP_API int sailor_hip_sky_compose(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params,
                                          const float* dSky, int32_t skyWidth, int32_t skyHeight, const float* dSun, int32_t sunWidth, int32_t sunHeight,
                                          float* dOut, int32_t width, int32_t height, const SailorBand* band);
/* The whole cube for callers that do not time-slice it over eight frames (SkyNode.cpp:749-818): six sailor_hip_sky_env_face launches, then
 * sailor_hip_generate_mipmaps_cube (:800-801).  Every argument is checked before the first launch. */
SAILOR_HIP_API int sailor_hip_sky_env_cubemap(SailorHipContext* ctx, const float* cameraPosition3, const SailorSkyParams* params,
                                              float* dCube, int32_t size, int32_t levels);

/* ---- Sky, the clouds: what SkyNode::Process adds with m_cloudsDensity > 0 (SkyNode.cpp:565-731) -------------------------------------------------
 * sailor_amd/csrc/sky_clouds.hip's header lists the decisions; tests/clouds_ref.py restates the three kernels in NumPy float32 and they are held to
 * it bit for bit.  All planes 16-byte aligned; all entry points record only (no synchronisation, capturable); a refused call records nothing. */

/* Replaces: the draw "Clouds" (SkyNode.cpp:565-603), define CLOUDS = Sky.shader:386-595, :656-692, without DITHER and DISCARD_BY_DEPTH.
 *   frame  : currentTime, cameraZNearZFar, view, invProjection and cameraPosition are read;  params : scatteringSteps outside 0 .. 10 is refused
 *   dSky   : `skySampler`, the plane of sailor_hip_sky_fill, bilinear Repeat
 *   dWeatherMap : `cloudsMapSampler`, mapHeight x mapWidth RGBA8 texels (r first), bilinear Repeat
 *   dNoiseLow / dNoiseHigh : `cloudsNoiseLowSampler` / `cloudsNoiseHighSampler`, size^3 R8_UNORM bytes, x fastest, trilinear Repeat, base level only
 *   dNoise : `g_noiseSampler`, noiseHeight x noiseWidth decoded linear float4 texels (the plane the HBAO entry points take), nearest Repeat
 *   dLinearDepth : `linearDepth`, depthHeight x depthWidth floats, nearest
 *   dClouds: device out, height x width float4 (the node: min(w, h) / 2 squared); alpha = 1 - transmittance; ROW height - 1 IS THE TOP OF THE VIEW */
SAILOR_HIP_API int sailor_hip_sky_clouds(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params,
                                         const float* dSky, int32_t skyWidth, int32_t skyHeight,
                                         const uint8_t* dWeatherMap, int32_t mapWidth, int32_t mapHeight,
                                         const uint8_t* dNoiseLow, int32_t lowSize, const uint8_t* dNoiseHigh, int32_t highSize,
                                         const float* dNoise, int32_t noiseWidth, int32_t noiseHeight,
                                         const float* dLinearDepth, int32_t depthWidth, int32_t depthHeight,
                                         float* dClouds, int32_t width, int32_t height);
/* sailor_hip_sky_sun with `cloudsSampler` honoured (Sky.shader:707-715): where the bilinear clamp-to-edge fetch of the clouds' alpha at uvView.xy is
 * >= 0.5 (or NaN: uvView divides by its own w) the texel stays (0, 0, 0, 0); elsewhere it holds the bits of sailor_hip_sky_sun.
 * frame->projection is read as well. */
SAILOR_HIP_API int sailor_hip_sky_sun_clouds(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params,
                                             const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight, float* dSun, int32_t width, int32_t height);
/* Replaces: the draw "Blit Clouds" (SkyNode.cpp:722-731): Blit.shader (bilinear clamp-to-edge, no y flip) under EBlendMode::AlphaBlending
 * (VulkanPipileneStates.cpp:245-246): rgb = src.rgb * src.a + dst.rgb * (1 - src.a), a = src.a * src.a - dst.a * (1 - src.a), in place.
 *   dTarget : device in/out, float4 per pixel of the width x height target, the rows of `band` only (first row = band->fbRowBegin) */
SAILOR_HIP_API int sailor_hip_sky_blit_clouds(SailorHipContext* ctx, const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight,
                                              float* dTarget, int32_t width, int32_t height, const SailorBand* band);

/* ---- Sky, "Stars & Clouds": the star points before and the sun shafts after the clouds blit (SkyNode.cpp:692-747) -----------------------------------
 * sailor_amd/csrc/sky_stars.hip's header lists the decisions -- the reading of the EBlendMode::Multiply state among them --; tests/stars_ref.py restates
 * the kernels in NumPy float32 and they are held to it bit for bit.  Both work in place on the rows of `band` of the target (first row =
 * band->fbRowBegin), record only (no allocation, no synchronisation, capturable), and a refused call records nothing. */

/* Replaces: the draw "Sun Shafts" (SkyNode.cpp:733-739), SunShafts.shader:96-140 under EBlendMode::Multiply (VulkanPipileneStates.cpp:248-254), read as
 * rgb = Cs Cd + Cs (1 - Ad) + Cd (1 - As), a = As As - Ad Ad.  uvView and both early-outs are computed on the host; a fragment that returns early is
 * (0, 0, 0, 0) and is still blended, so the pass is recorded in every case.
 *   frame  : view and projection are read;  params : lightDirection, sunShaftsIntensity, sunShaftsDistance (outside 1 .. 1024: SAILOR_HIP_ERR_INVALID_ARGUMENT)
 *   dClouds: `cloudsSampler`, the plane of sailor_hip_sky_clouds, bilinear clamp-to-edge, the base level;  it must not overlap dTarget */
SAILOR_HIP_API int sailor_hip_sky_sun_shafts(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params,
                                             const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight,
                                             float* dTarget, int32_t width, int32_t height, const SailorBand* band);
/* Replaces: the point-list draw of the star mesh (SkyNode.cpp:694-720), Stars.shader under EBlendMode::Additive, gl_PointSize = 1, no depth test.
 * Stars that share a pixel are added in index order (Vulkan's primitive order): the same bits on every run, no float atomics.
 *   frame   : view, projection, invProjection, cameraPosition; viewportSize must equal (width, height)
 *   model16 : host, the push constant: sailor_host_sky_stars_model
 *   dPositions / dColors : device, count x 3 and count x 4 floats (sailor_host_sky_star_mesh), 16-byte aligned; count above 65 536 is refused
 *   dClouds : `cloudsSampler`; NULL = the cleared m_pCloudsTexture, alpha 0
 * Needs a workspace of sailor_hip_sky_stars_workspace_bytes(count) bound to the context beforehand (sailor_hip_sky_stars_bind_workspace: the caller's
 * device memory, 16-byte aligned, not owned, NULL unbinds); without one the call is refused.  The query returns 0 for a count it refuses. */
SAILOR_HIP_API size_t sailor_hip_sky_stars_workspace_bytes(int32_t count);
SAILOR_HIP_API int sailor_hip_sky_stars_bind_workspace(SailorHipContext* ctx, void* dWorkspace, size_t workspaceBytes);
SAILOR_HIP_API int sailor_hip_sky_stars(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* model16,
                                        const float* dPositions, const float* dColors, int32_t count,
                                        const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight,
                                        float* dTarget, int32_t width, int32_t height, const SailorBand* band);

/* ---- Bloom (round 9): the Bloom node, FrameGraph/BloomNode.cpp:21-144 -- the mip pyramid over `Main`, rewritten in place ----------------------
 * tests/golden/DefaultRenderer.renderer:296-304.  `Main` is a level-major chain of RGBA32F planes (level l = max(1, width >> l) x max(1, height >> l),
 * the layout HipGraphicsDriver::CreateRenderTarget allocates; the reference's levels are rgba16f -- nothing is rounded through half here).
 * The kernels restate ComputeBloomDownscale.shader:72-127 and ComputeBloomUpscale.shader:44-95 one IEEE operation at a time, their per-group fp32
 * source-texel arithmetic included (sailor_amd/csrc/bloom.hip lists the decisions); tests/bloom_ref.py is the NumPy restatement they equal bit for bit.
 * All of them record only (no allocation, no synchronisation, capturable).  Planes are 16-byte aligned. */

/* The node's parameters (DefaultRenderer.renderer:298-302: the .x of its four vec4): 16 bytes */
typedef struct SailorBloomParams {
    float threshold;
    float knee;
    float bloomIntensity;
    float dirtIntensity;
} SailorBloomParams;

/* Texels of the first `levels` levels of a width x height mip chain = the texel offset of level `levels` (0 for levels == 0 and for a bad argument) */
SAILOR_HIP_API size_t sailor_hip_mip_chain_texels(int32_t width, int32_t height, int32_t levels);
/* Replaces: one Dispatch of the downscale loop (BloomNode.cpp:110-115), ComputeBloomDownscale.shader:72-127: the 13-tap Karis-weighted filter of
 * level i into level i + 1, with quadratic_threshold (:21-35) when useThreshold is set (the node: i == 0 only, :101).
 *   threshold4 : host, the push constant u_threshold as the node packs it (sailor_host_bloom_push_constants)
 *   dst extents must be max(1, src >> 1); dSrc == dDst is refused */
SAILOR_HIP_API int sailor_hip_bloom_downscale(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst, int32_t dstWidth,
                                              int32_t dstHeight, const float* threshold4, int32_t useThreshold);
/* Replaces: one Dispatch of the upscale loop (BloomNode.cpp:135-140), ComputeBloomUpscale.shader:44-95: the 3 x 3 tent of level mipLevel added to level
 * mipLevel - 1, which is read, modified and written; at mipLevel == 1 the lens-dirt term (:88-92) is added as well.
 *   dDirt : `u_dirt_texture` as decoded linear RGBA32F texels (bilinear, Repeat).  NULL = no dirt term: an extension for hosts without the asset.
 *   src extents must be max(1, dst >> 1); dSrc == dDst is refused */
SAILOR_HIP_API int sailor_hip_bloom_upscale(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst, int32_t dstWidth,
                                            int32_t dstHeight, int32_t mipLevel, float bloomIntensity, float dirtIntensity, const float* dDirt, int32_t dirtWidth,
                                            int32_t dirtHeight);
/* Replaces: the GPU work of BloomNode::Process (BloomNode.cpp:95-141): levels - 1 downscales (threshold on the first), then levels - 1 upscales from
 * the smallest level up, over the chain whose level 0 is width x height.  levels < 2 is refused; every argument is checked before the first launch. */
SAILOR_HIP_API int sailor_hip_bloom(SailorHipContext* ctx, float* dChain, int32_t width, int32_t height, int32_t levels, const SailorBloomParams* params,
                                    const float* dDirt, int32_t dirtWidth, int32_t dirtHeight);

/* ---- RCCL exchange for split frames (only when the frame is split AND a consumer needs the global list) ----
 * `comm` is an ncclComm_t created by the host.  Collective 1: all-gather of one uint32 (band total) per rank.
 * Collective 2: all-gather of the padded band index segments (each rank contributes `segmentCapacity` uints). */
SAILOR_HIP_API int sailor_hip_allgather_u32(SailorHipContext* ctx, void* comm, const uint32_t* dSend, uint32_t* dRecv, size_t countPerRank);

/* The whole exchange of a split frame (the reference's single Dispatch at FrameGraph/LightCullingNode.cpp:74-77 fills ONE pair of
 * buffers, a split frame has one pair per band): every rank hands in the lists of its band (sailor_hip_band_for_rank(width, height, rank,
 * worldSize), as sailor_hip_light_cull left them) and gets the reference's global `lightsGrid` (tiles x {offset, num}) and `culledLights`
 * ([0] = sum of num, then the lists at the canonical offsets) -- three ncclAllGather on the context's stream (band total; index segments in slots
 * sized by sailor_hip_exchange_adapt from an earlier exchange's totals, or of the worst case; grid) and one stitch kernel that takes each band's global
 * base from the gathered totals on the device.  The call only RECORDS (round 6; round 5 read the gathered totals back and synchronised the stream to
 * size the second gather): nothing is read back, nothing waits, and it may be captured into a hipGraph.
 *   comm          : an ncclComm_t of `worldSize` ranks created by the host (RCCL over xGMI)
 *   dGlobalCulled : globalCapacity uints, 1 + tiles * 128 holds every result
 *   dWorkspace    : sailor_hip_exchange_workspace_size(width, height, worldSize) bytes, 256-byte aligned */
#define SAILOR_MAX_SPLIT 64
SAILOR_HIP_API size_t sailor_hip_exchange_workspace_size(int32_t width, int32_t height, int32_t worldSize);
SAILOR_HIP_API int sailor_hip_exchange_light_lists(SailorHipContext* ctx, void* comm, int32_t rank, int32_t worldSize, int32_t width, int32_t height,
                                                   const SailorLightsGrid* dBandGrid, const uint32_t* dBandCulled, SailorLightsGrid* dGlobalGrid,
                                                   uint32_t* dGlobalCulled, size_t globalCapacity, void* dWorkspace, size_t workspaceBytes);
/* The stitch alone, on gathered slots: dTotals[worldSize]; dSegments[worldSize][segmentCapacity] (band r's culledLights[1 ..]);
 * dGrids[worldSize][gridCapacity] (band r's lightsGrid as uint32 pairs, band-local offsets). */
SAILOR_HIP_API int sailor_hip_stitch_light_lists(SailorHipContext* ctx, int32_t width, int32_t height, int32_t worldSize, const uint32_t* dTotals,
                                                 const uint32_t* dSegments, size_t segmentCapacity, const uint32_t* dGrids, size_t gridCapacity,
                                                 SailorLightsGrid* dGlobalGrid, uint32_t* dGlobalCulled, size_t globalCapacity);

/* The same two with the split given explicitly: tileRowBounds[worldSize + 1], rank r's band = tile rows [bounds[r], bounds[r + 1]) (bounds[0] = 0,
 * bounds[worldSize] = tile rows of the frame, non-decreasing) -- equal bands, cost-balanced bands (sailor_hip_band_from_tile_rows), anything in
 * between -- and with the capacity of dGlobalGrid in tiles (the stitch writes one entry per tile of the frame: fewer is an error, not an overrun).
 * The entry points above are these with the bounds of sailor_hip_band_for_rank and a grid of exactly the frame's tiles.  culledLights[0] is clamped
 * to what was written (globalCapacity - 1) when the segments did not fit. */
SAILOR_HIP_API size_t sailor_hip_exchange_workspace_size_rows(int32_t width, int32_t height, int32_t worldSize, const int32_t* tileRowBounds);
SAILOR_HIP_API int sailor_hip_exchange_light_lists_rows(SailorHipContext* ctx, void* comm, int32_t rank, int32_t worldSize, int32_t width, int32_t height,
                                                        const int32_t* tileRowBounds, const SailorLightsGrid* dBandGrid, const uint32_t* dBandCulled,
                                                        SailorLightsGrid* dGlobalGrid, size_t globalGridTiles, uint32_t* dGlobalCulled, size_t globalCapacity,
                                                        void* dWorkspace, size_t workspaceBytes);
SAILOR_HIP_API int sailor_hip_stitch_light_lists_rows(SailorHipContext* ctx, int32_t width, int32_t height, int32_t worldSize, const int32_t* tileRowBounds,
                                                      const uint32_t* dTotals, const uint32_t* dSegments, size_t segmentCapacity, const uint32_t* dGrids,
                                                      size_t gridCapacity, SailorLightsGrid* dGlobalGrid, size_t globalGridTiles, uint32_t* dGlobalCulled,
                                                      size_t globalCapacity);

/* The slot size of the exchange's second gather.  A context starts with the worst case (tiles of the largest band x 128 indices per rank: 16.7 MB gathered
 * per rank at C3 / 8 ranks for ~3 MB of lists).  sailor_hip_exchange_adapt is the exchange's one SYNCHRONISING call (like sailor_hip_context_synchronize):
 * it waits for the last exchange recorded through `ctx` -- its own event, not the stream's later work -- reads the three status words that exchange's
 * stitch kernel left in pinned host memory, and sizes the next exchange's slots from the largest band total it gathered (+ 25 %, whole 256-byte lines).
 * If that exchange was CLIPPED -- a band's total had outgrown a slot sized from an earlier frame: its global lists are incomplete -- *outClipped is 1, the
 * context's error text says which, and the next exchange goes back to the worst case.  The totals are the same on every rank, so the slot sizes are too,
 * PROVIDED every rank of the communicator calls this at the same point of its call sequence (the HIP backend: in front of every exchange but the first).
 * sailor_hip_exchange_set_slot_words sets the size explicitly (0 = the worst case).  Outputs may be NULL. */
SAILOR_HIP_API int sailor_hip_exchange_adapt(SailorHipContext* ctx, uint32_t* outLargestBandTotal, int32_t* outClipped, size_t* outSlotWords);
SAILOR_HIP_API int sailor_hip_exchange_set_slot_words(SailorHipContext* ctx, size_t slotWords);

/* ---- host-side math of the path (pure CPU, no device needed) ----------------------------------------------- */
/* Math/Math.cpp:18-21 PerspectiveRH (reversed Z) */
SAILOR_HIP_API int sailor_host_perspective_rh(float fovRadians, float aspect, float zNear, float zFar, float* outMat4);
/* glm::inverse(mat4) as used at ECS/CameraECS.cpp:20,33 */
SAILOR_HIP_API int sailor_host_mat4_inverse(const float* m, float* outMat4);
SAILOR_HIP_API int sailor_host_mat4_mul(const float* a, const float* b, float* outMat4);
/* Math/Transform.cpp:39-42 */
SAILOR_HIP_API int sailor_host_transform_matrix(const SailorTransform* t, float* outMat4);
/* FrameGraph/RHIFrameGraph.cpp:60-67 FillFrameData from a camera world matrix + lens */
SAILOR_HIP_API int sailor_host_fill_frame_data(const float* cameraWorld, float fovDegrees, float aspect, float zNear, float zFar,
                                               int32_t viewportWidth, int32_t viewportHeight, float currentTime, float deltaTime,
                                               SailorUboFrameData* outFrame);
/* Math/Bounds.cpp:142-193 Frustum::ExtractFrustumPlanes(world, aspect, fovY[deg], zNear, zFar): 6 planes, 8 corners (may be NULL) */
SAILOR_HIP_API int sailor_host_extract_frustum_planes(const float* worldMatrix, float aspect, float fovYDegrees, float zNear, float zFar,
                                                      float* outPlanes24, float* outCorners24);
/* FrameGraph/ShadowPrepassNode.cpp:387-404 + Math/Bounds.cpp:78-109 + ECS/LightingECS.cpp:292: the 4 lightsMatrices */
/* Math/Bounds.cpp:20-67 Frustum::ExtractFrustumPlanes(projectionViewMatrix) (+ CalculateCorners :110-140, reversed Z): planes L R T B N F, 8 corners */
SAILOR_HIP_API int sailor_host_extract_frustum_planes_matrix(const float* projectionViewMatrix, float* outPlanes24, float* outCorners24);
SAILOR_HIP_API int sailor_host_csm_matrices(const float* lightView, const float* cameraWorld, float aspect, float fovYDegrees,
                                            float cameraNear, float cameraFar, float* outMatrices64);
/* ECS/LightingECS.cpp:163-172: pack one light (cutOff in degrees -> cosines) */
SAILOR_HIP_API int sailor_host_pack_light(uint32_t type, uint32_t shadowType, const float* worldPosition, const float* direction,
                                          const float* intensity, const float* attenuation, const float* cutOffDegrees, const float* bounds,
                                          SailorLightShaderData* outLight);

/* FrameGraph/SkyNode.h:50-67: the member initialisers of SkyNode::SkyParams */
SAILOR_HIP_API int sailor_host_sky_params_default(SailorSkyParams* outParams);
/* FrameGraph/SkyNode.cpp:487-495: the view matrix of cube face 0..5 (glm::rotate about Math::vec3_Up / vec3_Right), PerspectiveRH(radians(90), 1,
 * 0.1, 1000) and its inverse, as the node writes them into the faces' frame data (:502-508) */
SAILOR_HIP_API int sailor_host_sky_face_matrices(int32_t face, float* outView16, float* outProjection16, float* outInvProjection16);
/* Sky.shader:247-264 CalculateSunColor(sunDirection) in fp32 (pow(x, 0.5) = sqrt, pow(x, 3) = (x x) x): the colour the cloud march multiplies in, which
 * does not vary per texel.  The march passes -dirToSun = normalize(lightDirection.xyz). */
SAILOR_HIP_API int sailor_host_sky_sun_color(const float* sunDirection3, float* outColor3);

/* FrameGraph/SkyNode.cpp:47-58: the node's temperature table from the `colors` rows of StarsColor.yaml (11 floats each: K, CMF, x, y, P, R, G, B, r, g, b):
 * row (K / 100 - 10), clamped to 0 .. 390, takes (R, G, B); later rows overwrite earlier ones.  outTable: 391 x 3 floats, zero where no row lands. */
SAILOR_HIP_API int sailor_host_sky_star_color_table(const float* rows, uint32_t rowCount, float* outTable);
/* FrameGraph/SkyNode.cpp:61-91 with Core/Utils.cpp:454-464 and SkyNode.cpp:836-875: the BSC5 bytes (a packed 28-byte header, then abs(starCount) packed
 * 32-byte entries) -> positions (x, y, z) and colours (r, g, b, a), pow(c, 1 / 2.2) applied.  sailor_amd/csrc/host_math.cpp lists the decisions where the
 * reference indexes out of range.  *outCount = the catalogue's star count; a catalogue shorter than its header or than the entries it counts, or a
 * capacity below the count, is SAILOR_HIP_ERR_INVALID_ARGUMENT and nothing is written past `capacity` stars. */
SAILOR_HIP_API int sailor_host_sky_star_mesh(const uint8_t* catalogue, size_t bytes, const float* table, float* outPositions, float* outColors,
                                             uint32_t capacity, uint32_t* outCount);
/* FrameGraph/SkyNode.cpp:208-211 and :698: translate(mat4(1), cameraPosition) * toMat4(precession), the star draw's push constant */
SAILOR_HIP_API int sailor_host_sky_stars_model(const float* cameraPosition3, float* outMat4);

/* FrameGraph/BloomNode.cpp:89-93: PushConstantsDownscale::m_threshold = (threshold, threshold - knee, 2 knee, 0.25 knee) -- as the node writes it: the
 * shader's comment expects knee * 0.25 to be a quotient's denominator; restated, not repaired */
SAILOR_HIP_API int sailor_host_bloom_push_constants(float threshold, float knee, float* outThreshold4);

/* FrameGraph/EyeAdaptationNode.cpp:154-170: the push constants of the node's two Dispatches for a width x height HDR target */
SAILOR_HIP_API int sailor_host_eye_adaptation_constants(int32_t width, int32_t height, float deltaTime, SailorEyeAdaptationConstants* outConstants);

/* Math/Bounds.cpp:211-243 Frustum::OverlapsSphere / ContainsSphere (scalar): sphere4 = (centre.xyz, radius); 1 / 0, negative = bad argument.
 * OverlapsSphere: no plane has the whole sphere behind it.  ContainsSphere: the sphere lies in front of all six planes by at least its radius. */
SAILOR_HIP_API int sailor_host_overlaps_sphere(const float* planes24, const float* sphere4);
SAILOR_HIP_API int sailor_host_contains_sphere(const float* planes24, const float* sphere4);
/* ECS/LightingECS.cpp:209-260 LightingECS::GetLightsInFrustum over flat component arrays (type, shadowType, active flag or NULL = all active,
 * owner position, bounds): shadow-casting directional lights in component order; point and spot lights whose sphere (radius = largest bound)
 * is contained in the frustum, sorted by distance to the camera with the reference's lower_bound insertion (equal distances: the later
 * component goes in front).  Every output array needs room for numLights entries. */
SAILOR_HIP_API int sailor_host_lights_in_frustum(const float* planes24, const float* cameraPosition3, uint32_t numLights, const uint32_t* types,
                                                 const uint32_t* shadowTypes, const uint8_t* active, const float* positions3, const float* bounds3,
                                                 uint32_t* outDirectional, uint32_t* outNumDirectional,
                                                 uint32_t* outPoint, float* outPointDistance, uint32_t* outNumPoint,
                                                 uint32_t* outSpot, float* outSpotDistance, uint32_t* outNumSpot);

/* The change tracking of LightingECS::PrepareCSMPasses (ECS/LightingECS.cpp:299-366) on the cascade overlap sets that
 * sailor_hip_csm_caster_masks produces.  SailorCsmSnapshots is LightingECS::m_csmSnapshots; SailorCsmView the transform half of a
 * CSMLightState (:14-38): light component index, camera position / rotation (xyzw), light position / rotation. */
typedef struct SailorCsmView {
    uint32_t componentIndex;
    float cameraPosition[4], cameraRotation[4], lightPosition[4], lightRotation[4];
} SailorCsmView;
typedef struct SailorCsmSnapshots SailorCsmSnapshots; /* opaque */
SAILOR_HIP_API SailorCsmSnapshots* sailor_host_csm_snapshots_create(void);
SAILOR_HIP_API SailorCsmSnapshots* sailor_host_csm_snapshots_clone(const SailorCsmSnapshots* snapshots);
SAILOR_HIP_API void sailor_host_csm_snapshots_destroy(SailorCsmSnapshots* snapshots);
SAILOR_HIP_API uint32_t sailor_host_csm_snapshots_count(const SailorCsmSnapshots* snapshots);
SAILOR_HIP_API int sailor_host_csm_snapshot_get(const SailorCsmSnapshots* snapshots, uint32_t index, uint32_t capacity, uint32_t* outCount, uint32_t* outMeshes,
                                                uint64_t* outFrames, int32_t* outHasView, SailorCsmView* outView);
/* One directional light: for cascade k = 0 .. numCascades-1 (snapshot slots firstSnapshot + k)
 *   * drop from its overlap set every mesh that an EARLIER cascade of the same shadow type, re-rendered this frame, overlaps (:310-327);
 *   * re-render it iff its (mesh, frame the mesh last changed) list differs from the stored snapshot, or -- with `view` -- the camera moved more
 *     than 15 units / turned past dot(forward, forward') = 0.9995 / the light moved at all since that snapshot was TAKEN (a kept snapshot keeps
 *     its old camera, :353-357).
 * overlapMasks / outMasks: numCascades x ceil(numEntities / 64) words; outRender: numCascades flags; lastChangedFrame: one per entity. */
SAILOR_HIP_API int sailor_host_csm_plan_passes(SailorCsmSnapshots* snapshots, uint32_t firstSnapshot, uint32_t numCascades, uint32_t numEntities,
                                               const uint64_t* overlapMasks, const uint32_t* shadowTypes, const uint64_t* lastChangedFrame,
                                               const SailorCsmView* view, uint32_t* outRender, uint64_t* outMasks);

/* ---- RenderScene: the surface pass (surface.hip; the Masked queue: surface_masked.hip, below) ---------------------------------------------------------------------------------------------
 * Replaces: the vertex stage of Content/Shaders/Standard.shader:126-139, the rasteriser between the stages and the material half of its fragment
 * stage (:379-389, :438) for the draws of FrameGraph/RenderSceneNode.cpp -- it PRODUCES the three planes sailor_hip_shade* consume.
 * The rasterisation rules are the depth prepass's (sailor_hip_raster_depth_camera: near-plane cut, 1/256-pixel snapping, 64-bit edge functions,
 * top-left rule, optional back-face cull, z = (z0 + (z1 - z0) w1) + (z2 - z0) w2, fragments outside (0, 1] do not exist), so the depth of the pass is
 * bit for bit the prepass's.  Depth test GreaterOrEqual (RHI/Types.h:536-537) in Vulkan's primitive order: a fragment wins its pixel if its z is
 * greater than what is stored, or equal and it is drawn later -- kept order-free as a 64-bit key per pixel, depthBits << 32 | (order + 1) under an
 * unsigned maximum, order = primBase + d * 2 * numTriangles + 2 * triangle + part (d = the instance's position in the draw, part = the half of a
 * triangle the near plane cut in two); low word 0 = no primitive.  Varyings are perspective-correct: l_k = float(e_k) / area, q_k = l_k / w_k,
 * s = (q0 + q1) + q2, b_k = q_k / s, a = (a0 b0 + a1 b1) + a2 b2; a vertex cut on the near plane gets a = aI + (aO - aI) t with the position's t.
 * texture() is the base level, bilinear, Repeat over RGBA8 texels; SAILOR_TEXTURE_SRGB decodes r, g, b per tap through sailor_host_srgb_table before
 * filtering.  The implicit mip selection of texture() (a descriptor with levels > 1): the `_lod` entry points of the mip-mapped section below; every entry
 * point of this section, of the Masked, glTF and indirect sections ignores SailorTextureDesc.levels and reads level 0.  NOT reproduced: anisotropy.
 * (Standard_glTF.shader: the glTF section below.)  A sampler index >= numTextures reads descriptor 0 (the reference binds g_defaultSampler there), a materialInstance >=
 * numMaterials reads material 0, a descriptor without texels samples as 0: no fetch leaves a table.
 * All entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves a text in last_error. */

/* RHI/Types.h:720-727 VertexP3N3T3B3UV2C4, interleaved, 72 bytes */
typedef struct SailorVertexP3N3T3B3UV2C4 {
    float texcoord[2];
    float position[3];
    float normal[3];
    float tangent[3];
    float bitangent[3];
    float color[4];
} SailorVertexP3N3T3B3UV2C4;
/* The vertex input of ShadowCaster.shader:46-59 is inPosition alone: dPositions[v] = dVertices[v].position, numVertices packed vec3 -- what
 * sailor_hip_raster_depth takes as dPositions -- for the shadow passes of meshes that live in a scene's interleaved vertex buffer.  Records only. */
SAILOR_HIP_API int sailor_hip_shadow_extract_positions(SailorHipContext* ctx, const SailorVertexP3N3T3B3UV2C4* dVertices, uint32_t numVertices,
                                                       float* dPositions);

/* Standard.shader:164-178 MaterialData, std430: 80 bytes */
typedef struct SailorMaterialData {
    float albedo[4];
    float ambient[4];
    float emission[4];
    float metallic;
    float roughness;
    float ao;
    uint32_t albedoSampler;
    uint32_t metalnessSampler;
    uint32_t normalSampler;
    uint32_t roughnessSampler;
    uint32_t _pad;
} SailorMaterialData;

/* one entry of Standard.shader:124 textureSamplers[]: a width x height RGBA8 image, one uint32 per texel (r in the low byte), row 0 first */
#define SAILOR_TEXTURE_SRGB 1u /* R8G8B8A8_SRGB (TextureAssetInfo.h:31, the default); without it UNORM (normal maps, ModelImporter.cpp:176) */
typedef struct SailorTextureDesc {
    const uint32_t* texels; /* device */
    int32_t width;
    int32_t height;
    uint32_t flags;
    uint32_t levels;        /* the mip levels behind `texels`, clamped to 1 .. floor(log2(max(width, height))) + 1 (0 reads as 1): the mip-mapped section below;
                               read by the `_lod` entry points only */
} SailorTextureDesc;

/* one DrawIndexed of RenderSceneNode.cpp (BindVertexBuffer / BindIndexBuffer / DrawIndexed): the draw kernel stores it into slot drawIndex of the
 * workspace, from where the resolve finds a key's draw by its primBase.  Slots are used in rising order with rising primBase. */
#define SAILOR_SURFACE_CULL_BACK 1u /* ECullMode::Back, frontFace counter-clockwise, as SAILOR_RASTER_CULL_BACK */
#define SAILOR_SURFACE_ALPHA_CUTOUT 2u /* the ALPHA_CUTOUT permutation of Standard.shader: sailor_hip_surface_draw_masked only, sailor_hip_surface_draw refuses it */
typedef struct SailorSurfaceDraw {
    const SailorVertexP3N3T3B3UV2C4* dVertices; /* device, already offset by vertexOffset */
    const uint32_t* dIndices;                   /* device, 3 x numTriangles, already offset by firstIndex */
    const uint32_t* dInstanceIds;               /* device, numDrawn instance indices in drawing order, or NULL for firstInstance .. firstInstance + numDrawn - 1 */
    uint32_t numTriangles;
    uint32_t numDrawn;
    uint32_t primBase;                          /* the order of the draw's first primitive: the previous draw's primBase + its sailor_hip_surface_draw_prims */
    uint32_t flags;                             /* SAILOR_SURFACE_CULL_BACK; SAILOR_SURFACE_ALPHA_CUTOUT through sailor_hip_surface_draw_masked, _draw_gltf, _draw_indirect, _msaa_draw and _msaa_draw_gltf only; SAILOR_SURFACE_GLTF (below) through _draw_gltf, _draw_indirect and _msaa_draw_gltf only; SAILOR_SURFACE_BLEND_* (the Transparent section) through _peel_draw, _peel_draw_gltf, _bucket_draw and _bucket_draw_gltf only */
    uint32_t firstInstance;
    uint32_t _pad;
} SailorSurfaceDraw;

/* the workspace of one pass over the rows of `band`: a header, the sRGB table, one 64-bit key per pixel of the band, maxDraws descriptors; 0 = invalid */
SAILOR_HIP_API size_t sailor_hip_surface_workspace_bytes(int32_t width, int32_t height, const SailorBand* band, uint32_t maxDraws);
/* where the keys begin in a workspace: uint64 per pixel of the band, row-major, depthBits << 32 | (order + 1) (tests and diagnostics) */
SAILOR_HIP_API size_t sailor_hip_surface_keys_offset(void);
/* Replaces: BeginRenderPass(Main, DepthBuffer) at RenderSceneNode.cpp.  Keys = prepass depth bits << 32 (dDepthOrNull: the raw width x height depth
 * attachment of the WHOLE frame, as sailor_hip_raster_depth_camera leaves it), or 0; every descriptor slot empty. */
SAILOR_HIP_API int sailor_hip_surface_begin(SailorHipContext* ctx, const float* dDepthOrNull, int32_t width, int32_t height, const SailorBand* band,
                                            void* dWorkspace, size_t workspaceBytes);
/* Replaces: one DrawIndexed with Standard.shader's vertex stage (:128-131) and the fixed-function rasteriser: k_surface_visibility. */
SAILOR_HIP_API int sailor_hip_surface_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                           const SailorPerInstanceData* dInstances, uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band,
                                           void* dWorkspace, size_t workspaceBytes);
/* Replaces: the varyings (:132-138) and the material half of the fragment stage (:382-389, :438) at the winning fragment of every pixel: k_surface_resolve.
 *   dSurface : device out, 3 planes of float4, each the band's rows x width, planeStride float4 apart (what sailor_hip_shade* read):
 *              P0 = worldPosition, albedo.a; P1 = normal, roughness; P2 = albedo.rgb, metallic; an uncovered pixel gets 0, (0, 0, 1, 1), 0
 *   dDepthOutOrNull : device out, the band's rows x width floats: the final depth (equal to the prepass depth wherever the same draws were prepassed)
 *   dCoverageOrNull : device out, the band's rows x width bytes: 1 where a primitive of this pass owns the pixel */
SAILOR_HIP_API int sailor_hip_surface_resolve(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances,
                                              const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                              int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace, size_t workspaceBytes,
                                              float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull);
/* Replaces: the colour writes of the pass over what `Blit Sky -> Main` left: target = covered ? radiance : target (both the band's rows x width float4). */
SAILOR_HIP_API int sailor_hip_surface_composite(SailorHipContext* ctx, const float* dRadiance, const void* dWorkspace, size_t workspaceBytes, float* dTarget,
                                                int32_t width, int32_t height, const SailorBand* band);
/* The sRGB transfer function (c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4, c = i / 255) in double, rounded once to fp32. */
SAILOR_HIP_API int sailor_host_srgb_table(float out[256]);
/* numDrawn * 2 * numTriangles (saturating at 2^64 - 1): what a draw adds to the running primBase.  sailor_hip_surface_draw refuses a draw whose primBase + this reaches 2^32 - 1. */
SAILOR_HIP_API int sailor_hip_surface_draw_prims(uint32_t numTriangles, uint32_t numDrawn, uint64_t* out);

/* ---- The Masked render queue: ALPHA_CUTOUT in the surface pass (surface_masked.hip) ----------------------------------------------------------
 * Replaces: the `Tag: Masked` draws of FrameGraph/RenderSceneNode.cpp and of FrameGraph/DepthPrepassNode.cpp.  A glTF material with alphaMode == "MASK"
 * (AssetRegistry/Model/ModelImporter.cpp:213-229) gets the render queue Masked, the define ALPHA_CUTOUT and IsRequiredCustomDepthShader() == true; a
 * material that requires a custom depth shader is its own depth material (DepthPrepassNode.cpp:86-90, :107-115, :246-255), so the Masked prepass runs
 * Standard.shader with ALPHA_CUTOUT against no colour attachment, and a discarded fragment writes no depth.  RenderSceneNode.cpp applies the same tag
 * filter with colour and depth writes.  Standard.shader:383 `material.albedo = material.albedo * texture(textureSamplers[material.albedoSampler],
 * vin.texcoord) * vin.color`, :403-408 `if (material.albedo.a < 0.5) discard;`.
 * Pinned:
 *  1. The tested value is alpha = (mat.albedo[3] * tA.w) * a[8], in exactly the operation order of k_surface_resolve.  tA.w is the bilinear Repeat
 *     fetch of the albedo sampler's alpha (never sRGB-decoded); a[8] is the perspective-correct vertex colour alpha; a[0], a[1] (the texcoord) and a[8]
 *     are interpolated by the formula above: l_k = float(e_k) / area, q_k = l_k / w_k, s = (q0 + q1) + q2, b_k = q_k / s, a = (a0 b0 + a1 b1) + a2 b2; a
 *     vertex cut on the near plane is aI + (aO - aI) t.  So at every pixel a cutout draw owns, the resolve's P0.w is, bit for bit, the alpha the draw tested.
 *  2. A fragment is discarded iff alpha < 0.5f.  A NaN alpha survives, as in GLSL.
 *  3. The look-up rules of the resolve hold for the alpha fetch: a materialInstance >= numMaterials reads material 0, a sampler index >= numTextures reads
 *     descriptor 0, a descriptor without texels samples 0 (so everything finite is discarded).
 *  4. A discarded fragment does not exist: it writes no key and no depth and takes no part in ties.  Discard is a pure function of the fragment, so the
 *     keys stay order-free; the decision is taken in the draw, before the key is issued (exact inside test and z -> plain load of the pixel's key -> alpha
 *     only if the key would win -> atomicMax only for a survivor).  sailor_hip_surface_resolve, _composite and sailor_hip_surface_draw are unchanged.
 *  5. NOT reproduced: masked shadow casters.  (The Transparent queue has its own section, below; Standard_glTF.shader's alphaCutoff as a material field is
 *     sailor_hip_surface_draw_gltf's, below: the threshold HERE is the constant 0.5.)  (A Masked prepass is begin(opaque depth), the masked draws, sailor_hip_surface_store_depth: what the runtime
 *     mirror's DepthPrepass node records through DrawIndexedIndirect.)
 * Both entry points record only; a refused call launches nothing and leaves its text in last_error. */

/* Replaces: one DrawIndexed of a material with or without ALPHA_CUTOUT: k_surface_visibility_masked.  The checks and refusals of sailor_hip_surface_draw;
 * flags may also hold SAILOR_SURFACE_ALPHA_CUTOUT, which requires dMaterials / dTextures (the tables sailor_hip_surface_resolve gets) to be present.  Without
 * the flag the keys are sailor_hip_surface_draw's and the tables are not read. */
SAILOR_HIP_API int sailor_hip_surface_draw_masked(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                  const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                  const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                  const SailorBand* band, void* dWorkspace, size_t workspaceBytes);
/* Replaces: the depth writes of a pass that held cutout draws (a Masked DepthPrepass; a z-writing RenderScene pass): k_surface_store_depth writes the
 * high word of every key of the band into the band's rows of dDepth, the raw width x height depth attachment of the WHOLE frame. */
SAILOR_HIP_API int sailor_hip_surface_store_depth(SailorHipContext* ctx, const void* dWorkspace, size_t workspaceBytes, float* dDepth, int32_t width,
                                                  int32_t height, const SailorBand* band);

/* ---- glTF materials: Standard_glTF.shader in the surface pass (surface_gltf.hip) -------------------------------------------------------------------
 * Replaces: Content/Shaders/Standard_glTF.shader, the shader AssetRegistry/Model/ModelImporter.cpp:156-231 gives every imported model, where it differs from
 * Standard.shader: the vertex stage's tangentBasis (:136-138), MaterialData (:42-58), the material half of the fragment stage (:389-396), the emissive
 * term (:399, :432) and the ALPHA_CUTOUT threshold (:411).  The light loop, CalculateLighting and AmbientLighting are Standard.shader's under other field
 * names, so the shade kernels are unchanged: this section PRODUCES their inputs (the three planes, the `ao` plane of SailorIblDesc) and adds the emissive
 * term behind them.  A pass may mix both shaders; the flag of the draw that owns a pixel decides.
 * Pinned:
 *  1. One material table.  SailorGltfMaterialData is the std430 image of :42-58 and has SailorMaterialData's 80-byte array stride, so `dMaterials` stays ONE
 *     array of 80-byte slots (the engine's single material SSBO); a slot is read as SailorGltfMaterialData by a draw that carries SAILOR_SURFACE_GLTF and as
 *     SailorMaterialData by one that does not.  A materialInstance >= numMaterials reads slot 0 as the record of the draw that asks.
 *  2. The position transform (:130-133) is Standard.shader's: a glTF draw without ALPHA_CUTOUT issues sailor_hip_surface_draw's keys bit for bit.
 *  3. ALPHA_CUTOUT: rules 1-4 of the masked section with alpha = (baseColorFactor[3] * tA.w) * a[8], tA fetched through baseColorSampler, and a fragment
 *     discarded iff alpha < alphaCutoff -- one fp32 compare: a NaN on either side survives, alphaCutoff == 0 discards nothing (not even alpha 0, nor -0).
 *  4. tangentBasis: varyings 9..17 of a vertex are N * (T | B | Nv) column by column, (N[0] a0 + N[1] a1) + N[2] a2 with N[c] the columns of
 *     N = transpose(inverse(mat3(model))), m[c][r] = model[4 c + r], inverse in glm's 3 x 3 form, one rounding per written operation:
 *       det = + m00 (m11 m22 - m21 m12) - m10 (m01 m22 - m21 m02) + m20 (m01 m12 - m11 m02)        (left to right), oneOverDet = 1.0f / det
 *       I00 = + (m11 m22 - m21 m12) oneOverDet   I10 = - (m10 m22 - m20 m12) oneOverDet   I20 = + (m10 m21 - m20 m11) oneOverDet
 *       I01 = - (m01 m22 - m21 m02) oneOverDet   I11 = + (m00 m22 - m20 m02) oneOverDet   I21 = - (m00 m21 - m20 m01) oneOverDet
 *       I02 = + (m01 m12 - m11 m02) oneOverDet   I12 = - (m00 m12 - m10 m02) oneOverDet   I22 = + (m00 m11 - m10 m01) oneOverDet
 *     N[c][r] = I[r][c].  A singular model gives non-finite normals; they pass through.  Every other varying and the interpolation are the surface pass's.
 *  5. The fetches of a glTF pixel, each the surface pass's texture() under its descriptor's own sRGB flag (ModelImporter leaves orm, occlusion and emissive
 *     textures at the sRGB default and only the normal map UNORM; no special case here): tA (baseColorSampler), tO (ormSampler; ONE fetch, .z and .y used),
 *     tOcc = .x of occlusionSampler, tE (emissiveSampler), tN (normalSampler).
 *       P0 = (worldPosition, (baseColorFactor[3] tA.w) a[8])       P2 = ((baseColorFactor[k] tA.k) a[5 + k], metallicFactor tO.z)      P1.w = roughnessFactor tO.y
 *       n = normalize(2 tN - 1) as in the surface pass, then n *= normalScale on all three components, then P1.xyz = normalize(tangentBasis * n)
 *       emissive = (emissiveFactor[k] tE.k for k = 0..2, tOcc)          (emissiveFactor[3] is not read)
 *       aoOut = (tOcc < aoIn) ? tOcc : aoIn        GLSL's min(x, y) = y < x ? y : x with x = g_AO (:392).  A NaN aoIn stays NaN; a NaN tOcc leaves aoIn.
 *     The SSBO's occlusionStrength is overwritten at :392 and never read.
 *  6. A pixel owned by a draw without SAILOR_SURFACE_GLTF gets sailor_hip_surface_resolve's three planes bit for bit, emissive (0, 0, 0, 1) and aoOut = aoIn's
 *     bits; an uncovered pixel the same.  aoIn is 1.0f everywhere if dAoInOrNull is NULL.
 *  7. The composite adds the emissive term behind the shade: rgb = emissive.rgb + radiance.rgb, one fp32 add per channel.  The reference sums
 *     ((emissive + ao ambient) + L1) + ...; the shade has formed fma(ambient, ao, sum L) already, so this is ONE re-association, inside the shade's bound.
 * NOT reproduced: masked shadow casters.  (The Transparent queue, alphaMode BLEND: its own section, below.)
 * All entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves its text in last_error. */

/* Standard_glTF.shader:42-58 MaterialData, std430: two vec4 (0, 16), five floats (32..48), five uints (52..68), padded to the vec4 alignment: 80 bytes */
typedef struct SailorGltfMaterialData {
    float baseColorFactor[4];
    float emissiveFactor[4];
    float metallicFactor;
    float roughnessFactor;
    float occlusionStrength;
    float normalScale;
    float alphaCutoff;
    uint32_t baseColorSampler;
    uint32_t normalSampler;
    uint32_t ormSampler;
    uint32_t occlusionSampler;
    uint32_t emissiveSampler;
    uint32_t _pad[2];
} SailorGltfMaterialData;

#define SAILOR_SURFACE_GLTF 4u /* the draw's material is Standard_glTF.shader's: sailor_hip_surface_draw_gltf and _draw_indirect only; sailor_hip_surface_draw and _draw_masked refuse it */

/* Replaces: one DrawIndexed of a Standard_glTF.shader material, with or without ALPHA_CUTOUT: k_surface_visibility_gltf.  The arguments, checks and refusals
 * of sailor_hip_surface_draw_masked; flags must hold SAILOR_SURFACE_GLTF and may hold CULL_BACK and ALPHA_CUTOUT; the descriptor is stored with the flag,
 * from where sailor_hip_surface_resolve_gltf reads it.  dMaterials: the one table of rule 1. */
SAILOR_HIP_API int sailor_hip_surface_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                const SailorBand* band, void* dWorkspace, size_t workspaceBytes);
/* Replaces: sailor_hip_surface_resolve for a pass that may hold glTF draws: k_surface_resolve_gltf.  Its arguments, and
 *   dAoInOrNull  : device, the band's rows x width floats: g_AO at the pixel (what the shade's SailorIblDesc.ao would be); NULL = 1.0f
 *   dAoOutOrNull : device out, the band's rows x width floats: rule 5's aoOut, what the shade reads as SailorIblDesc.ao instead; may be dAoInOrNull itself
 *   dEmissive    : device out, float4 per pixel of the band: rule 5's emissive, for sailor_hip_surface_composite_gltf */
SAILOR_HIP_API int sailor_hip_surface_resolve_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances,
                                                   const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                                   int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace, size_t workspaceBytes,
                                                   float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull,
                                                   const float* dAoInOrNull, float* dAoOutOrNull, float* dEmissive);
/* Replaces: sailor_hip_surface_composite for such a pass: target = covered ? (emissive.rgb + radiance.rgb, radiance.a) : target (rule 7). */
SAILOR_HIP_API int sailor_hip_surface_composite_gltf(SailorHipContext* ctx, const float* dRadiance, const float* dEmissive, const void* dWorkspace,
                                                     size_t workspaceBytes, float* dTarget, int32_t width, int32_t height, const SailorBand* band);

/* ---- GPU-driven draws: DrawIndexedIndirect in the surface pass (surface_indirect.hip) ---------------------------------------------------------------
 * Replaces: the scene draws as the reference records them -- every one a DrawIndexedIndirect (RHI/Batch.hpp:169, :289; RHI/GraphicsDriver.h:323;
 * VulkanGraphicsDriver.cpp:2607-2620 issues drawCount > 1 one command at a time), whose command the "GPU Culling" dispatch (Batch.hpp:174-190,
 * ComputeMeshCulling.shader:146-177 == sailor_hip_mesh_cull_compact[_ex]) has rewritten on the device: instanceCount is the number of survivors and the
 * per-instance records of the batch are compacted in place behind firstInstance.  The host never learns the count; the draw reads it where it runs.
 * Pinned:
 *  1. `draw` is the command AS THE HOST WROTE IT (Batch.hpp:148-153): dVertices and dIndices already offset by vertexOffset / firstIndex, numTriangles from
 *     indexCount, numDrawn the CAPACITY -- the un-culled instanceCount.  The grid and the primBase arithmetic are sized from it.  dInstanceIds must be NULL
 *     (refused otherwise); draw->firstInstance is ignored.
 *  2. The kernel reads two words of *dCommand when it RUNS, with plain loads: instanceCount and firstInstance.  Nothing of *dCommand is read at record
 *     time, so a captured graph replays against whatever the buffer holds then.
 *  3. Drawn instances: n = min(instanceCount, capacity, numInstanceRecords - firstInstance), and n = 0 when firstInstance >= numInstanceRecords.  Instance
 *     d < n is record firstInstance + d; no fetch leaves a table.  A lane whose d >= n does not exist: no set-up, no part in the ballots of the
 *     large-triangle path.  A block whose every lane is beyond n leaves after the one uniform load (block 0 stays: it stores the descriptor).
 *  4. The descriptor stored in slot drawIndex holds numDrawn = n and firstInstance as read, so sailor_hip_surface_resolve[_gltf], _composite[_gltf] and
 *     _store_depth work unchanged.  A command with n == 0 still leaves its descriptor.
 *  5. order = primBase + d * 2 * numTriangles + 2 * triangle + part as in every draw of the pass.  The NEXT draw's primBase advances by the capacity:
 *     sailor_hip_surface_draw_prims(numTriangles, capacity).  Order only has to be monotone, so the winners are those of direct draws of the survivors; the
 *     low words of the keys differ from such a pass's where a draw behind a partially counted one owns the pixel.  The 2^32 - 1 refusal is checked against
 *     the capacity.
 *  6. The slices of a draw of few triangles (gridDim.y) are chosen from the capacity: a draw of large capacity and few survivors runs its large triangles
 *     unsliced.  What that costs has not been measured.
 *  7. flags: SAILOR_SURFACE_CULL_BACK; SAILOR_SURFACE_ALPHA_CUTOUT (requires the tables); SAILOR_SURFACE_GLTF picks k_surface_visibility_indirect_gltf,
 *     its absence k_surface_visibility_indirect.  Without ALPHA_CUTOUT the keys are sailor_hip_surface_draw's and the tables are not read.
 *  8. Checks and refusals: those of sailor_hip_surface_draw_masked / _gltf, plus dCommand NULL or not 4-byte aligned, plus dInstanceIds != NULL.
 * NOT reproduced -- a DECISION: indexCount, firstIndex and vertexOffset are taken from the host's copy (`draw`), not from *dCommand.  The reference's host
 * wrote them in the same frame and no GPU pass of the reference rewrites them.  Also not reproduced: indirect shadow casters, drawCount > 1 in one call
 * (the caller loops, as the Vulkan driver does).
 * The call records only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves its text in last_error. */

/* Replaces: one command of DrawIndexedIndirect (RHI/GraphicsDriver.h:323; VulkanGraphicsDriver.cpp:2607-2620 issues drawCount > 1 one by one). */
SAILOR_HIP_API int sailor_hip_surface_draw_indirect(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                    const SailorDrawIndexedIndirectData* dCommand, const SailorPerInstanceData* dInstances,
                                                    uint32_t numInstanceRecords, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                    const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                    const SailorBand* band, void* dWorkspace, size_t workspaceBytes);

/* ---- Mip-mapped material textures: chain generation and the implicit level of detail (texture_mips.hip, surface_lod.hip) ------------------------------
 * Replaces: TextureAssetInfo.h:34 (m_bShouldGenerateMips = true), TextureImporter.cpp:247-295 (mipLevels = floor(log2(max(w, h))) + 1),
 * VulkanCommandBuffer.cpp:814-907 (the chain, built by 2:1 VK_FILTER_LINEAR blits) and VulkanSamplers.cpp:37-40 (mipmapMode LINEAR, mipLodBias 0, minLod 0,
 * maxLod 64): every texture(textureSamplers[...], vin.texcoord) of Standard.shader and Standard_glTF.shader is a trilinear fetch at an implicit level of
 * detail, the one behind ALPHA_CUTOUT included.  Vulkan leaves the scale factor partly to the implementation.  Pinned:
 *  1. The chain.  A descriptor has n = clamp(levels, 1, full) levels, full = floor(log2(max(width, height))) + 1 in integers, levels == 0 reads as 1.  Level l
 *     has max(width >> l, 1) x max(height >> l, 1) texels and begins sailor_hip_mip_chain_texels(width, height, l) uint32 texels behind `texels`.
 *  2. Generation, level l + 1 from level l, per channel: decode the byte (r, g, b through sailor_host_srgb_table under SAILOR_TEXTURE_SRGB; alpha and
 *     unflagged channels as byte / 255.0f), filter with sailor_hip_blit_linear's tap set (bilinear_taps at ((x + 0.5) / wd, (y + 0.5) / hd), lerp2: for even
 *     extents the 2 x 2 mean with weights of exactly 0.5), encode: sRGB -> the number of entries of sailor_host_srgb_encode_table that are <= x; UNORM ->
 *     (uint)floorf(x * 255.0f + 0.5f).
 *  3. Derivatives.  For pixel (i, j), j the framebuffer row, uv(X, Y) = (a[0], a[1]) of the surface pass's varying formula for the owning part's set-up,
 *     evaluated with the exact integer edge functions at the centre (256 X + 128, 256 Y + 128) whether or not that centre lies in the triangle or the frame
 *     (Vulkan's helper invocations).  Fine derivatives inside the quad at (i & ~1, j & ~1), one fp32 subtraction each:
 *       d/dx = uv(i | 1, j) - uv(i & ~1, j)           d/dy = uv(i, j | 1) - uv(i, j & ~1)
 *     A pure function of (the owning primitive's set-up, the pixel): keys stay order-free, a band needs no neighbour rows.
 *  4. Scale factor, per descriptor (its own w, h), one rounding per written operation:
 *       ax = dudx * float(w), bx = dvdx * float(h), rx = ax * ax + bx * bx;  ay = dudy * float(w), by = dvdy * float(h), ry = ay * ay + by * by;
 *       r2 = ry > rx ? ry : rx
 *  5. Level selection: !(r2 > 1.0f) -> level 0 alone (magnification, zero, NaN); else r2 >= 4^(n-1) -> level n - 1 alone (+inf); else
 *       lambda = 0.5f * canonical_log2f(r2), hi = (int)lambda; hi >= n - 1 -> level n - 1 alone; else delta = lambda - float(hi), lo = hi + 1 and per channel
 *       t = t_hi * (1.0f - delta) + t_lo * delta
 *     with each t_l the surface pass's base-level fetch (repeat_tap, lerp2, sRGB per tap) over level l's extents.  n == 1 is that fetch bit for bit; no
 *     derivative is formed.  A descriptor without texels samples 0.
 *  6. ALPHA_CUTOUT through the `_lod` draws tests alpha with tA.w fetched by rules 3-5 through the albedo / base-colour sampler, in the draw, before the key is
 *     issued; the neighbour centres' edge functions are affine steps of the fragment's own (exact).  At every pixel such a draw owns,
 *     sailor_hip_surface_resolve_lod's P0.w is, bit for bit, the alpha that was tested.  Without ALPHA_CUTOUT the keys are sailor_hip_surface_draw's.
 * NOT reproduced: anisotropy (maxAnisotropy = 8 is implementation-defined), textureLod and bias, the UI and particle textures, formats other than RGBA8, the
 * Transparent queue at an implicit level of detail (its draws and resolves read level 0).
 * All device entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves its text in last_error. */

/* floor(log2(max(width, height))) + 1 by integer operations; 0 for an extent outside 1 .. 32768 */
SAILOR_HIP_API uint32_t sailor_hip_texture_mip_levels(int32_t width, int32_t height);
/* out[k - 1] = the sRGB transfer function of (k - 0.5) / 255 in double, rounded once to fp32, k = 1 .. 255: the byte of x is the number of entries <= x */
SAILOR_HIP_API int sailor_host_srgb_encode_table(float out[255]);
/* Replaces: GenerateMipMaps for one 2-D RGBA8 image (VulkanCommandBuffer.cpp:814-907): k_texture_mip_down, one launch per level, in place.  dTexels holds
 * level 0 and room for sailor_hip_mip_chain_texels(width, height, levels) texels; flags = SAILOR_TEXTURE_SRGB or 0.  Refused: dTexels NULL or not 4-byte
 * aligned, an extent outside 1 .. 32768, levels outside 1 .. sailor_hip_texture_mip_levels(width, height), unknown flag bits. */
SAILOR_HIP_API int sailor_hip_texture_generate_mips(SailorHipContext* ctx, uint32_t* dTexels, int32_t width, int32_t height, uint32_t levels, uint32_t flags);
/* sailor_hip_surface_resolve_gltf with every fetch (four of a Standard pixel, five of a glTF pixel) by rules 3-5: k_surface_resolve_lod.  Its arguments,
 * checks and refusals; a pass of either or both shaders. */
SAILOR_HIP_API int sailor_hip_surface_resolve_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances,
                                                  const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                                  int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace, size_t workspaceBytes,
                                                  float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull,
                                                  const float* dAoInOrNull, float* dAoOutOrNull, float* dEmissive);
/* sailor_hip_surface_draw_masked / _draw_gltf with rule 6: k_surface_visibility_lod, or k_surface_visibility_lod_gltf if the draw carries SAILOR_SURFACE_GLTF
 * (optional here).  Their arguments, checks and refusals. */
SAILOR_HIP_API int sailor_hip_surface_draw_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                               const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                               const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                               const SailorBand* band, void* dWorkspace, size_t workspaceBytes);
/* sailor_hip_surface_draw_indirect with rule 6: k_surface_visibility_indirect_lod[_gltf].  Its arguments, checks and refusals. */
SAILOR_HIP_API int sailor_hip_surface_draw_indirect_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                        const SailorDrawIndexedIndirectData* dCommand, const SailorPerInstanceData* dInstances,
                                                        uint32_t numInstanceRecords, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                        const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                        const SailorBand* band, void* dWorkspace, size_t workspaceBytes);

/* ---- The Transparent render queue: ordered blended draws in the surface pass (surface_transparent.hip) -------------------------------------------
 * Replaces: a RenderScene node with `Tag: Transparent` (FrameGraph/RenderSceneNode.cpp filters proxies by any tag).  ModelImporter.cpp:213-229 gives a glTF
 * material with alphaMode == "BLEND" the render queue Transparent, depth test on and z-write OFF; MaterialImporter.cpp:329-357 lets a .mat file choose
 * blendMode from None / Additive / AlphaBlending / Multiply; VulkanPipileneStates.cpp:236-254 holds the blend states.  A transparent pass is a list of
 * draws, each of Standard or Standard_glTF, issued in the host's order against the depth attachment the prepass and the opaque passes left.
 * Pinned:
 *  1. A fragment exists iff it does in the Masked section (set-up, near-plane cut, snap, cull, top-left rule, fill) AND passes z >= depth[pixel], compared
 *     as the uint32 images of two non-negative floats -- what the surface pass's depth test does against a key seeded by sailor_hip_surface_begin; equal
 *     depth passes -- AND, under SAILOR_SURFACE_ALPHA_CUTOUT, survives the discard rule of its shader.  A discarded fragment occupies no layer.  The depth
 *     attachment is READ ONLY: depth is never written.
 *  2. The fragments of a pixel are blended in ascending primitive order, the orderPlus1 = primBase + 2 (instance * numTriangles + triangle) + part + 1 the
 *     keys carry: within a draw instance, then triangle, then the part the near plane made; across draws the order they were issued in.  Depth plays no
 *     part in the order.
 *  3. The source colour of a fragment: src.rgb = what the shade kernels produce from the three planes sailor_hip_surface_resolve / _resolve_gltf give if
 *     that fragment owns the pixel, plus -- when an emissive plane is passed -- emissive.rgb exactly as sailor_hip_surface_composite_gltf adds it
 *     (emissive.k + radiance.k).  src.a = the resolve's P0.w bit for bit (outColor.a = material.albedo.a, Standard.shader:438).  The tile's light lists,
 *     g_AO and the shadow maps are the opaque pass's: the reference culls lights against the prepass depth too, so a transparent fragment in front of it sees
 *     that tile's list.  Reproduced, not fixed.
 *  4. The blend, per draw, from SAILOR_SURFACE_BLEND_* in the draw's flags; one fp32 rounding per written operation, no contraction; the source products
 *     first, then the destination's, then the add or the subtract:
 *       NONE     : dst = src, all four channels (what ModelImporter gives a BLEND material: an overwrite without depth write)
 *       ADDITIVE : dst = src + dst, all four channels
 *       ALPHA    : dst.rgb = src.rgb * src.a + dst.rgb * (1 - src.a);  dst.a = src.a * src.a - dst.a * (1 - src.a)    (the alpha op is SUBTRACT)
 *       MULTIPLY : SAILOR_HIP_ERR_UNSUPPORTED for scene draws (VK_BLEND_OP_MULTIPLY_EXT: the decision recorded for the sun shafts stands)
 *     A fragment with src.a == 0 still blends; NaN and Inf pass through.
 *  5. The target is the RGBA32F Main plane, as for every other pass; this queue stays single-sampled (the Multisampled section lists it as not reproduced).
 * Mechanism: the pass is peeled by primitive order.  Layer k holds, at each pixel, that pixel's k-th fragment in primitive order:
 *   sailor_hip_surface_peel_begin (zero keys; `last` zeroed for layer 0 only) -> every draw through _peel_draw / _peel_draw_gltf (a fragment of rule 1 with
 *   orderPlus1 > last[pixel] issues (0xFFFFFFFF - orderPlus1) << 32 | zbits by plain load and atomicMax: the maximum is the smallest order beyond the previous
 *   layer, order-free) -> _peel_commit (a non-zero key becomes zbits << 32 | orderPlus1, last[pixel] = orderPlus1, the committed pixels are added to *dCount)
 *   -> the workspace is an ordinary surface workspace: sailor_hip_surface_resolve / _resolve_gltf (dDepthOutOrNull = NULL) and the shade, unchanged ->
 *   sailor_hip_surface_blend.  A pass of L layers is L such rounds and one more { begin, draws, commit } whose count is the OVERFLOW: the pixels that still
 *   had a fragment left.  Every layer rasterises the pass again.  Indirect draws and the `_lod` fetch are not part of this section.
 * All entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves its text in last_error. */
#define SAILOR_SURFACE_BLEND_SHIFT 3u /* SailorSurfaceDraw.flags bits 3-4: the draw's EBlendMode; accepted by sailor_hip_surface_peel_draw / _peel_draw_gltf and _bucket_draw / _bucket_draw_gltf only */
#define SAILOR_SURFACE_BLEND_MASK 3u
#define SAILOR_SURFACE_BLEND_NONE 0u
#define SAILOR_SURFACE_BLEND_ADDITIVE 1u
#define SAILOR_SURFACE_BLEND_ALPHA 2u
#define SAILOR_SURFACE_BLEND_MULTIPLY 3u /* refused: SAILOR_HIP_ERR_UNSUPPORTED */

/* Begins one layer: sailor_hip_surface_begin without a depth (zero keys, empty descriptor slots, the sRGB table).
 *   dLast     : device, the band's rows x width uint32: the orderPlus1 each pixel committed last (0: none)
 *   startPass : non-zero zeroes dLast (layer 0 of a pass); 0 leaves it (every later layer and the overflow round) */
SAILOR_HIP_API int sailor_hip_surface_peel_begin(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                                                 size_t workspaceBytes, uint32_t* dLast, int32_t startPass);
/* One DrawIndexed of a transparent pass: k_surface_peel.  The arguments, checks and refusals of sailor_hip_surface_draw_masked; flags may also hold a blend
 * mode (MULTIPLY: SAILOR_HIP_ERR_UNSUPPORTED).  Every layer issues the same draws with the same drawIndex and primBase.
 *   dDepth : device, the raw width x height depth attachment of the WHOLE frame (as sailor_hip_surface_store_depth takes it); read only
 *   dLast  : as above; read only here */
SAILOR_HIP_API int sailor_hip_surface_peel_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth, const uint32_t* dLast);
/* The same for a Standard_glTF.shader material: k_surface_peel_gltf; flags must hold SAILOR_SURFACE_GLTF, as for sailor_hip_surface_draw_gltf. */
SAILOR_HIP_API int sailor_hip_surface_peel_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                     const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                     const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                     const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth, const uint32_t* dLast);
/* Ends a layer's draws: k_surface_peel_commit.  *dCount (device, uint32) += the pixels of the band that committed a fragment; the caller zeroes it. */
SAILOR_HIP_API int sailor_hip_surface_peel_commit(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                                                  size_t workspaceBytes, uint32_t* dLast, uint32_t* dCount);
/* Rule 4 at every pixel the committed layer owns: k_surface_blend.  dRadiance: the shade's output; dSurfaceP0: the first plane of the resolve's surface (its
 * .w is src.a); dEmissiveOrNull: sailor_hip_surface_resolve_gltf's emissive plane, or NULL for a pass resolved by sailor_hip_surface_resolve; all float4 per
 * pixel of the band, as dTarget.  A pixel without a fragment keeps the target's bits. */
SAILOR_HIP_API int sailor_hip_surface_blend(SailorHipContext* ctx, const float* dRadiance, const float* dSurfaceP0, const float* dEmissiveOrNull,
                                            const void* dWorkspace, size_t workspaceBytes, float* dTarget, int32_t width, int32_t height, const SailorBand* band);

/* -- Per-pixel fragment buckets: the Transparent queue in ONE rasterisation (surface_buckets.hip) --
 * A SECOND MECHANISM under the same rules: 1 to 5 above are untouched, and so are the peel's entry points, which remain the default route of every caller.
 * The draws run once and leave, at every pixel, the pixel's first K fragments in primitive order; every layer is then read out of that store instead of being
 * rasterised again, and goes through the same resolve, the same shade and sailor_hip_surface_blend.  A layer read out is the key the peel's commit would have
 * left, so the two routes give the same bits.
 * The store: K + 1 planes of uint64 over the band's rows, plane-major -- bucket[p][row * width + x], p = 0 .. K.  A slot holds orderPlus1 << 32 | zbits, or
 * EMPTY, all ones (never a key: an order that would reach 2^32 - 1 is refused).  After the draws plane p holds the pixel's (p + 1)-th smallest orderPlus1
 * among the fragments that exist by rule 1, or EMPTY; plane K is the sentinel, non-empty exactly where the pixel has more than K fragments.  The insertion
 * is order-free, 64-bit atomicMin alone (surface_masked_body.h has the argument).  (K + 1) x 8 bytes a pixel.
 * A pass: _bucket_begin -> every draw once through _bucket_draw / _bucket_draw_gltf -> K times { _bucket_layer(k), sailor_hip_surface_resolve /
 * _resolve_gltf (dDepthOutOrNull = NULL), the shade, sailor_hip_surface_blend } -> _bucket_layer(K), whose count is the OVERFLOW, equal to the peel's by
 * definition.  Indirect draws and the `_lod` fetch are not part of this sub-section either.
 * All entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves its text in last_error.
 * Refused everywhere: layers outside 1 .. 64; a NULL or not 8-byte aligned dBuckets; bucketBytes below sailor_hip_surface_bucket_bytes. */
/* The bytes of the store of `layers` (= K) layers over the band's rows: (layers + 1) * fbRowCount * width * 8.  0 on a bad argument (a NULL band, a width or
 * a row count outside 1 .. 32768, layers outside 1 .. 64). */
SAILOR_HIP_API size_t sailor_hip_surface_bucket_bytes(int32_t width, const SailorBand* band, uint32_t layers);
/* Begins a pass: sailor_hip_surface_begin without a depth (zero keys, empty descriptor slots, the sRGB table) and every slot of the store EMPTY. */
SAILOR_HIP_API int sailor_hip_surface_bucket_begin(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                                                   size_t workspaceBytes, void* dBuckets, size_t bucketBytes, uint32_t layers);
/* One DrawIndexed of the pass, issued ONCE: k_surface_bucket.  The arguments, checks and refusals of sailor_hip_surface_peel_draw (MULTIPLY:
 * SAILOR_HIP_ERR_UNSUPPORTED) with the store in place of dLast.  The workspace takes the draw's descriptor, for the resolves and the blend. */
SAILOR_HIP_API int sailor_hip_surface_bucket_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                  const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                  const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                  const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth, void* dBuckets,
                                                  size_t bucketBytes, uint32_t layers);
/* The same for a Standard_glTF.shader material: k_surface_bucket_gltf; flags must hold SAILOR_SURFACE_GLTF. */
SAILOR_HIP_API int sailor_hip_surface_bucket_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                       const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                       const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width,
                                                       int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth,
                                                       void* dBuckets, size_t bucketBytes, uint32_t layers);
/* Reads layer k out of the store: k_surface_bucket_layer.  k < layers: every key of the workspace becomes plane k's fragment as zbits << 32 | orderPlus1 (0
 * where the slot is EMPTY) -- an ordinary surface workspace, as behind sailor_hip_surface_peel_commit -- and *dCount (device, uint32; the caller zeroes it)
 * += the pixels that have one.  k == layers: the workspace is left alone and *dCount += the pixels whose sentinel slot is taken, the OVERFLOW.
 * Also refused: k > layers; a NULL or not 4-byte aligned dCount. */
SAILOR_HIP_API int sailor_hip_surface_bucket_layer(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                                                   size_t workspaceBytes, const void* dBuckets, size_t bucketBytes, uint32_t layers, uint32_t k,
                                                   uint32_t* dCount);

/* ---- Multisampled RenderScene pass: per-sample keys, shaded layers, the AVERAGE resolve (surface_msaa.hip) ------------------------------------------
 * Replaces: the multisampled targets of the scene pass.  Sailor.cpp:150 creates the renderer with EMsaaSamples::Samples_8; VulkanCommandBuffer.cpp:341-386
 * puts every pass whose material supports multisampling (the default) on the driver's cached MSAA colour and depth targets and resolves both with
 * VK_RESOLVE_MODE_AVERAGE_BIT (:287-298).  VulkanPipileneStates.cpp:141-149 has sampleShadingEnable = VK_FALSE and alphaToCoverageEnable = VK_FALSE, and no
 * varying of Standard.shader or Standard_glTF.shader is `centroid`: coverage and depth are per sample, the fragment shader runs once per pixel and primitive
 * with its varyings at the pixel centre, `discard` removes the whole fragment.
 * OPT-IN: no existing entry point, kernel or default changes; a pass that is not multisampled keeps the single-sample entries.  Pinned:
 *  1. Sample positions: Vulkan's standard sample locations, in 1/256 pixel from the pixel's top-left corner, exact on the rasteriser's grid.
 *     S = 1: (128,128).  S = 2: (192,192), (64,64).  S = 4: (96,32), (224,96), (32,160), (160,224).
 *     S = 8: (144,80), (112,176), (208,144), (80,48), (48,208), (16,112), (176,240), (240,16).
 *     Any other count is refused (the reference's 16 / 32 / 64 have no standard table restated here).  sailor_host_msaa_sample_positions returns the table.
 *  2. Coverage of sample s of pixel (i, j) by a set-up triangle (the surface pass's vertices, near-plane cut, snap and cull, unchanged): the three edge
 *     functions at (256 i + sx, 256 j + sy), none negative, a value of 0 counting only on a top or left edge -- the surface pass's rule moved from the centre
 *     to the sample.  The box is every pixel that holds a sample inside the triangle's bounding box (the walk may visit more; they hold no covered sample).
 *     A triangle that covers samples but no pixel centre exists here.
 *  3. Depth of a covered sample: z0 + (z1 - z0) (float(e1) / area) + (z2 - z0) (float(e2) / area) with the SAMPLE's e1, e2 and the triangle's area; kept
 *     iff 0 < z <= 1.  With S = 1 the keys are sailor_hip_surface_draw_masked's, bit for bit.
 *  4. Discard (ALPHA_CUTOUT, both shaders) is evaluated once per pixel and primitive, by the Masked queue's rule with the edge functions of the pixel
 *     CENTRE; the centre may lie outside the triangle, and the barycentrics then extrapolate, as the hardware does without `centroid`.  A discarded fragment
 *     owns no sample.  Base-level fetch, as sailor_hip_surface_draw_masked.
 *  5. Store: one uint64 per sample, pixel-major -- store[(row * width + x) * S + s], row counted from the band's first -- holding zbits << 32 | orderPlus1
 *     under an unsigned maximum: GreaterOrEqual in primitive order, as the surface pass.  orderPlus1 == 0: no primitive of this pass.  S x 8 bytes a pixel
 *     (64 at S = 8: 531 MB for 3840 x 2160).  A fragment's order of work is the masked draw's, per pixel: a plain relaxed load per covered sample; the discard
 *     only if some sample would win; an atomic maximum only for the samples that would win.  The keys are order-free.
 *  6. Begin: keys = sampleDepthBits << 32 from an optional per-sample depth (floats in the store's layout: what a multisampled prepass stored through
 *     _msaa_store_depth), or 0.
 *  7. Layers: layer k of a pixel is its (k + 1)-th smallest distinct non-zero orderPlus1 among its S keys.  _msaa_layer(k), k < layers = L, 1 <= L <= S,
 *     writes an ordinary surface workspace key zbits << 32 | orderPlus1 -- the zbits of the lowest-numbered sample holding that order; 0 where the pixel has
 *     no such layer --, a weight byte w_k = the samples holding that order, adds the pixels that have the layer to a device counter and, for k = 0, writes a
 *     byte u = the samples that hold no order.  With L < S the samples whose order is not among the pixel's first L are CLIPPED: their number is added to
 *     w_(L-1) of that pixel, and the pixel is counted in a second device counter.  L = S never clips.  The read-out is stateless: it recomputes from the S
 *     keys and keeps no per-pixel cursor.
 *  8. Shading of a layer: the unchanged sailor_hip_surface_resolve / _resolve_gltf / _resolve_lod with dDepthOutOrNull = NULL, then the unchanged shade --
 *     the fragment shader at the pixel centre, once per primitive and pixel.
 *  9. Accumulate: the reference's AVERAGE resolve over what `Blit Sky -> Main` left in every sample.  c_k = what sailor_hip_surface_composite would store,
 *     or sailor_hip_surface_composite_gltf's (emissive.rgb + radiance.rgb, radiance.a) when an emissive plane is given.  The weights w / S are exact in fp32;
 *     every product and every sum is rounded on its own (no fused multiply-add); a term of weight 0 is omitted, not multiplied.
 *       k = 0: w_0 = 0: untouched.  w_0 = S: target = c_0, its bits.  Otherwise target = (u / S) target + (w_0 / S) c_0, the first term omitted when u = 0.
 *       k >= 1: w_k = 0: untouched.  Otherwise target = target + (w_k / S) c_k.
 *     Samples this pass does not own take the target's value at the pixel: exact when the target was uniform over each pixel's samples before the pass, the
 *     case behind the Sky blit.  SANCTIONED DIVERGENCE: a second pass over the edge pixels of an earlier multisampled pass; to be exact there, draw both
 *     queues into ONE store (the entries allow it: the orders of the second continue the first's).
 * 10. Depth out: the S sample depths (the keys' high words, in the store's layout) for the next pass's begin, and the resolved depth, the reference's
 *     AVERAGE (((z_0 + z_1) + ...) + z_(S-1)) * (1 / S) in fp32, into the band's rows of the whole-frame depth attachment.
 * A pass: _msaa_begin -> every draw once through _msaa_draw / _msaa_draw_gltf -> L times { _msaa_layer(k), a resolve, the shade, _msaa_accumulate(k) } ->
 * _msaa_store_depth where the pass writes depth.
 * NOT reproduced (a pass that needs one keeps the single-sample entries): the runtime mirror (HipGraphicsDriver, FrameGraph.cpp -- DepthPrepass, DebugDraw,
 * particles and the Transparent queue share the surface and would all have to follow); indirect draws and the `_lod` draw's alpha fetch (a layer may still
 * be resolved by sailor_hip_surface_resolve_lod); the Transparent queue; SAILOR_VULKAN_MSAA_IMPACTS_TEXTURE_SAMPLING (sample shading); 16 samples and more.
 * All entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing, leaves its text in last_error and leaves
 * store, workspace and outputs untouched.  Refused everywhere: samples outside {1, 2, 4, 8}; a NULL or not 16-byte aligned dStore; storeBytes below
 * sailor_hip_surface_msaa_bytes. */
/* The table of rule 1: out[s] = (sx, sy), s < samples.  SAILOR_HIP_ERR_INVALID_ARGUMENT for another count or a NULL out. */
SAILOR_HIP_API int sailor_host_msaa_sample_positions(uint32_t samples, int32_t out[][2]);
/* The bytes of the store over the band's rows: fbRowCount * width * samples * 8.  0 on a bad argument (a NULL band, a width or a row count outside
 * 1 .. 32768, samples outside {1, 2, 4, 8}). */
SAILOR_HIP_API size_t sailor_hip_surface_msaa_bytes(int32_t width, const SailorBand* band, uint32_t samples);
/* Begins a pass: rule 6 into the store (dSampleDepthOrNull: device, fbRowCount * width * samples floats, or NULL), and sailor_hip_surface_begin without a
 * depth into the workspace (zero keys, empty descriptor slots, the sRGB table).  Also refused: a misaligned dSampleDepthOrNull. */
SAILOR_HIP_API int sailor_hip_surface_msaa_begin(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                                                 size_t workspaceBytes, void* dStore, size_t storeBytes, uint32_t samples, const float* dSampleDepthOrNull);
/* One DrawIndexed of the pass: k_surface_msaa.  The arguments, checks and refusals of sailor_hip_surface_draw_masked (so the LOD, indirect and blend flags are
 * unknown flags here) plus the store.  The workspace takes the draw's descriptor, for the resolves. */
SAILOR_HIP_API int sailor_hip_surface_msaa_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                const SailorBand* band, void* dWorkspace, size_t workspaceBytes, void* dStore, size_t storeBytes,
                                                uint32_t samples);
/* The same for a Standard_glTF.shader material: k_surface_msaa_gltf; flags must hold SAILOR_SURFACE_GLTF, as for sailor_hip_surface_draw_gltf. */
SAILOR_HIP_API int sailor_hip_surface_msaa_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                                     const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials,
                                                     const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height,
                                                     const SailorBand* band, void* dWorkspace, size_t workspaceBytes, void* dStore, size_t storeBytes,
                                                     uint32_t samples);
/* Rule 7 for layer k: k_surface_msaa_layer.  dWeight, dUncoveredOrNull: device, a byte per pixel of the band; dCount, dClippedOrNull: device uint32, added
 * to (the caller zeroes them).  Also refused: layers outside 1 .. samples; k >= layers; a NULL dWeight; a NULL dUncoveredOrNull at k = 0; a NULL or
 * misaligned dCount; a misaligned dClippedOrNull. */
SAILOR_HIP_API int sailor_hip_surface_msaa_layer(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                                                 size_t workspaceBytes, const void* dStore, size_t storeBytes, uint32_t samples, uint32_t layers, uint32_t k,
                                                 uint8_t* dWeight, uint8_t* dUncoveredOrNull, uint32_t* dCount, uint32_t* dClippedOrNull);
/* Rule 9 for layer k: k_surface_msaa_accumulate.  dRadiance: the shade's output; dEmissiveOrNull: a glTF resolve's emissive plane, or NULL; dWeight,
 * dUncoveredOrNull: what _msaa_layer(k) wrote; all over the band's rows, as dTarget.  Also refused: k >= samples; a NULL dWeight; a NULL dUncoveredOrNull at
 * k = 0; a NULL or not 16-byte aligned colour plane. */
SAILOR_HIP_API int sailor_hip_surface_msaa_accumulate(SailorHipContext* ctx, const float* dRadiance, const float* dEmissiveOrNull, const uint8_t* dWeight,
                                                      const uint8_t* dUncoveredOrNull, uint32_t samples, uint32_t k, float* dTarget, int32_t width,
                                                      int32_t height, const SailorBand* band);
/* Rule 10: k_surface_msaa_store_depth.  dSampleDepthOutOrNull: device, fbRowCount * width * samples floats; dDepthOrNull: the raw width x height depth
 * attachment of the WHOLE frame.  Also refused: both NULL; a misaligned output. */
SAILOR_HIP_API int sailor_hip_surface_msaa_store_depth(SailorHipContext* ctx, const void* dStore, size_t storeBytes, uint32_t samples,
                                                       float* dSampleDepthOutOrNull, float* dDepthOrNull, int32_t width, int32_t height, const SailorBand* band);

/* ---- DebugDraw: the line-list pass of the Gizmo material (debug_lines.hip) ---------------------------------------------------------------------
 * Replaces: the draw FrameGraph/DebugDrawNode.cpp:19-79 replays -- RHI/DebugContext.cpp:382-398 (DrawDebugMesh: one DrawIndexed over the line list that
 * DrawLine :76-98 and the shapes :100-158 built) with Content/Shaders/Gizmo.shader under the material of DebugContext.cpp:272: LineList, lineWidth 1, depth
 * test and depth write, no bias, GREATER_OR_EQUAL, blend None.  The pass is sailor_hip_surface_begin(current DepthBuffer) -> sailor_hip_debug_lines_draw ->
 * sailor_hip_debug_lines_resolve; the key layout (depthBits << 32 | order + 1), the workspace and the fragment's depth test are the surface pass's.
 * Vulkan leaves non-strict line rasterisation partly to the implementation.  Pinned:
 *  1. Vertex stage: clip = viewProjection * vec4(position, 1), ((c0 x + c1 y) + c2 z) + c3 (Gizmo.shader:22); segment s has the vertices dIndices[2s],
 *     dIndices[2s + 1], or 2s, 2s + 1 without an index buffer (the identity DebugContext uploads).
 *  2. Clip, in clip space and fp32, against the distances w - z, w + x, w - x, w + y, w - y in this order, tIn = 0, tOut = 1: both ends < 0 rejects; one end
 *     < 0 gives t = dA / (dA - dB), which raises tIn (A outside) or lowers tOut (B outside); tIn > tOut rejects.  The clipped ends are computed from the
 *     ORIGINAL ends, P0 = tIn > 0 ? A + (B - A) tIn : A, P1 = tOut < 1 ? A + (B - A) tOut : B, for x, y, z, w and the four colour channels; an end with
 *     !(w > 0) rejects.  (The far plane is the per-fragment z > 0 of rule 5.)
 *  3. Snap: the surface pass's -- nx = x / w, xf = (nx + 1) (W 0.5), yf = (ny + 1) (H -0.5) + H, X = rintf(256 xf), rejected unless |256 xf| < 1e9.
 *  4. Coverage, exact in integers, closed-form per major-axis step: x-major iff |dX| >= |dY|; dX == dY == 0 has no fragment.  x-major, pixel centre
 *     M = 256 c + 128: column c has a fragment iff X0 <= M < X1 (dX > 0) or X1 < M <= X0 (dX < 0) -- start included, end excluded; its row is
 *     floor((Y0 dX + dY (M - X0)) / (256 dX)), an exact integer floor: the pixel that contains the line's point at that centre.  y-major is the mirror
 *     image.  A fragment outside the frame or the band's rows does not exist.
 *  5. Attributes: t = float(M - X0) / float(dX); z = z0 + (z1 - z0) t with z_k = z / w of the clipped ends (a line's depth is linear in screen space); a
 *     fragment exists only if z > 0 && z <= 1.  Colour is perspective-correct: q0 = (1 - t) / w0, q1 = t / w1, b = q1 / (q0 + q1), c = c0 + (c1 - c0) b, in
 *     exactly this operation order.
 *  6. Order: primBase + the segment's index; the larger key wins, so equal depth goes to the later segment, and a line at the seeded depth wins over it.
 *     Keys are order-free, so any distribution of the work gives the same bits.
 * All entry points record only (no allocation, no synchronisation, capturable); a refused call launches nothing and leaves its text in last_error.  One draw
 * per pass (DebugContext issues exactly one); a draw of no segments records nothing. */

/* RHI/Types.h VertexP3C4, interleaved, 28 bytes */
typedef struct SailorVertexP3C4 {
    float position[3];
    float color[4];
} SailorVertexP3C4;

/* DebugContext.cpp:393-397: BindVertexBuffer / BindIndexBuffer / DrawIndexed(numRenderedVertices, 1, 0, 0, 0) */
typedef struct SailorDebugLinesDraw {
    const SailorVertexP3C4* dVertices; /* device */
    const uint32_t* dIndices;          /* device, 2 x numSegments, or NULL: the identity */
    uint32_t numSegments;
    uint32_t primBase;                 /* the order of the first segment */
} SailorDebugLinesDraw;

/* Replaces: the DrawIndexed of DebugContext.cpp:397 up to the depth test: k_debug_lines_draw issues the keys of every fragment into a workspace that
 * sailor_hip_surface_begin seeded.  viewProjection: the push constant of :395, column-major.  Refused: a draw whose primBase + numSegments reaches 2^32 - 1. */
SAILOR_HIP_API int sailor_hip_debug_lines_draw(SailorHipContext* ctx, const float viewProjection[16], const SailorDebugLinesDraw* draw, int32_t width,
                                               int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes);
/* Replaces: Gizmo.shader:34 `outColor = fragColor` and the colour and depth writes of the pass: k_debug_lines_resolve writes, at every pixel a segment owns
 * (low word of the key != 0), all four channels of the colour into dTarget (the band's rows x width float4) and the key's depth into the band's rows of
 * dDepth, the raw width x height depth attachment of the WHOLE frame, as sailor_hip_surface_store_depth does.  Other pixels keep both. */
SAILOR_HIP_API int sailor_hip_debug_lines_resolve(SailorHipContext* ctx, const float viewProjection[16], const SailorDebugLinesDraw* draw, int32_t width,
                                                  int32_t height, const SailorBand* band, const void* dWorkspace, size_t workspaceBytes, float* dTarget,
                                                  float* dDepth);
/* numSegments: what the draw adds to a running primBase, by analogy with sailor_hip_surface_draw_prims. */
SAILOR_HIP_API int sailor_hip_debug_lines_prims(uint32_t numSegments, uint64_t* out);

/* ---- RenderImGui: ordered alpha-blended UI triangles (ui_draw.hip) ----------------------------------------------------------------------------
 * Replaces: the draws FrameGraph/RenderImGuiNode.cpp:21-60 replays -- Submodules/ImGuiApi.cpp:190-276 (ImGui_RenderDrawData: per draw list and per command a
 * scissor and one DrawIndexed) with Content/Shaders/ImGuiUI.shader under the material of ImGuiApi.cpp:295-332: TriangleList over VertexP2UV2C1, no depth test,
 * no depth write, no cull, one sample, EBlendMode::AlphaBlending, one RGBA8 UNORM texture (Linear, Repeat, one level).  The pass is ONE
 * sailor_hip_ui_draw over the flattened commands of the frame (sailor_host_ui_flatten).  Pinned:
 *  1. Vertex fetch: SailorVertexP2UV2C1, 20 bytes, 4-byte aligned; a colour channel is c = (float)byte / 255.0f, r in the low byte.  Indices are 16-bit or
 *     32-bit (indexBytes of the draw).  Triangle k of a command has the indices firstIndex + 3k .. + 2 and the vertices vertexOffset + index; an index
 *     position outside the index buffer or a vertex outside [0, numVertices) drops its triangle: no fetch leaves a buffer.  indexCount % 3 trailing indices
 *     are ignored.
 *  2. Vertex stage and viewport (ImGuiUI.shader, ImGuiApi.cpp:108-113): nx = px * scale.x + translate.x -- two fp32 roundings, no fused multiply-add --, ny
 *     likewise; xf = (nx + 1.0f) * ((float)W * 0.5f), yf = (ny + 1.0f) * ((float)H * 0.5f).  The viewport's height is positive: no flip, row 0 is the top.
 *  3. Rasterisation is the depth prepass's after projection: X = rintf(xf * 256.0f), a triangle with !(|xf * 256| < 1e9) on any coordinate (NaN included) is
 *     dropped; 64-bit integer edge functions at the pixel centre (256 i + 128, 256 j + 128), the top-left rule, both windings drawn (a winding swap
 *     exchanges vertices 1 and 2 WITH their colour and uv), zero area dropped.  No near-plane cut (z = 0, w = 1); no depth test, read or write.
 *  4. Scissor: pixel (i, j) belongs to a command iff scissor[0] <= i < scissor[0] + scissor[2] and scissor[1] <= j < scissor[1] + scissor[3];
 *     sailor_host_ui_flatten computes offset and extent in fp32 exactly as ImGuiApi.cpp:236-252 does (the extent is the truncated DIFFERENCE).  A zero
 *     extent that survived the float test draws nothing.
 *  5. Varyings: w = 1, so interpolation is affine: l_k = float(e_k) / area, a = (a0 l0 + a1 l1) + a2 l2 for the four colour channels and both texcoords.
 *     This is the surface pass's order with q_k = l_k; DECISION: the surface pass's b_k = q_k / s is not applied (s is 1 up to rounding; the rule above
 *     is the whole formula).
 *  6. Texture: the surface pass's fetch of a SailorTextureDesc without SAILOR_TEXTURE_SRGB -- base level, bilinear, Repeat, RGBA8 texels as UNORM, no sRGB
 *     decode.  One texture per pass (ImGuiApi.cpp:255-262).  A descriptor without texels samples as 0.  DECISION: a descriptor WITH SAILOR_TEXTURE_SRGB is
 *     refused rather than silently read as UNORM.
 *  7. Fragment and blend (VulkanPipileneStates.cpp:245-246), one IEEE rounding per written operation, in place on an fp32 RGBA plane:
 *        src = colour * texel (per channel);  rgb = src.rgb * src.a + dst.rgb * (1.0f - src.a);  a = src.a * src.a - dst.a * (1.0f - src.a)
 *     (the alpha op is SUBTRACT).  Triangles blend in command order, then index order within a command -- Vulkan's primitive order --, and a pixel's result is
 *     that sequential chain bit for bit.  A fragment with src.a == 0 still blends (the alpha line changes dst.a).
 *  8. NOT reproduced: the reference's attachment is B8G8R8A8_SRGB -- its hardware blends in linear light and re-quantises to 8 bits after every fragment;
 *     BackBuffer here is an fp32 plane (as sailor_hip_debug_view leaves it) and keeps the unquantised chain.  MSAA does not apply (bSupportMultisampling is
 *     false).  User textures per command (the reference has none).
 *  9. sailor_hip_ui_draw only records: no allocation, no synchronisation, capturable.  A refused call launches nothing and leaves a text in last_error.
 *     Refused: a null or misaligned pointer, a non-positive extent, an index width other than 2 or 4, a command range outside the index buffer, a workspace
 *     smaller than the size query's answer, a scissor outside the target (negative offset or extent, or offset + extent beyond width / height), more than
 *     SAILOR_UI_MAX_COMMANDS commands.
 * DECISION (the cumulative triangle counts): the caller hands the commands twice, `commands` on the host and `dCommands`, the same array on the device.  The
 * host copy is what the call checks and sizes its launches from; the device copy is what the kernels read, and k_ui_scan computes the cumulative triangle
 * counts from it on the device.  The kernels bound every fetch by the buffer sizes themselves, so a device copy that differs from the host copy draws
 * something else but reads and writes nothing out of bounds. */

/* RHI/Types.h:656-661 VertexP2UV2C1, interleaved, 20 bytes; m_color is fetched as R8G8B8A8_UNORM (Renderer.cpp:78-82) */
typedef struct SailorVertexP2UV2C1 {
    float position[2];
    float uv[2];
    uint32_t color;
} SailorVertexP2UV2C1;

/* one DrawIndexed of ImGuiApi.cpp:265-270 under the SetViewport of :247-252: scissor = offset x, offset y, extent x, extent y */
typedef struct SailorUiCommand {
    uint32_t firstIndex;   /* IdxOffset + the lists before it */
    uint32_t indexCount;   /* ElemCount */
    int32_t vertexOffset;  /* VtxOffset + the lists before it */
    int32_t scissor[4];
} SailorUiCommand;

#define SAILOR_UI_MAX_COMMANDS 16384u

/* the workspace of one sailor_hip_ui_draw over at most numTriangles triangles (the sum of indexCount / 3 over the commands): the cumulative counts of
 * SAILOR_UI_MAX_COMMANDS commands and one set-up record per triangle.  It does not depend on the extent (the blend keeps its pixels in registers); width and
 * height are checked only.  *out = 0 and INVALID_ARGUMENT for a non-positive extent. */
SAILOR_HIP_API int sailor_hip_ui_workspace_bytes(uint32_t numTriangles, int32_t width, int32_t height, size_t* out);
/* Replaces: ImGui_RenderDrawData's draws and the blend of the pass: k_ui_scan (cumulative triangle counts), k_ui_setup (a lane per triangle: rules 1 to 4
 * into a record), k_ui_blend (a block per 32 x 32 pixels of the band: rules 3 to 7 in primitive order, one store per touched pixel).
 *   dVertices, numVertices : device, the merged vertex buffer      dIndices, indexBytes, numIndices : device, the merged index buffer, 2 or 4 bytes an index
 *   commands / dCommands   : host / device copies of the flat command array (see DECISION above)
 *   scale, translate       : the push constants of ImGuiApi.cpp:118-125       texture : host struct, copied at record time; texels on the device
 *   dTarget                : device, the band's rows x width float4, blended in place
 * A band's target holds its own rows only; a band without rows, a draw without commands or without triangles records nothing. */
SAILOR_HIP_API int sailor_hip_ui_draw(SailorHipContext* ctx, const SailorVertexP2UV2C1* dVertices, uint32_t numVertices, const void* dIndices, uint32_t indexBytes,
                                      uint32_t numIndices, const SailorUiCommand* commands, const SailorUiCommand* dCommands, uint32_t numCommands,
                                      const float scale[2], const float translate[2], const SailorTextureDesc* texture, void* dWorkspace, size_t workspaceBytes,
                                      float* dTarget, int32_t width, int32_t height, const SailorBand* band);

/* ImDrawData as plain data, for sailor_host_ui_flatten: per list its buffer sizes and commands, per command what ImDrawCmd holds */
#define SAILOR_UI_CALLBACK_NONE 0u
#define SAILOR_UI_CALLBACK_RESET 1u /* ImDrawCallback_ResetRenderState: re-issues the set-up state, draws nothing */
#define SAILOR_UI_CALLBACK_USER 2u  /* any other UserCallback: draws nothing */
typedef struct SailorUiDrawCmd {
    float clipRect[4];   /* ImDrawCmd::ClipRect: x1, y1, x2, y2 */
    uint32_t elemCount;
    uint32_t idxOffset;
    uint32_t vtxOffset;
    uint32_t callback;   /* SAILOR_UI_CALLBACK_* */
} SailorUiDrawCmd;
typedef struct SailorUiDrawList {
    uint32_t vtxCount;   /* VtxBuffer.Size */
    uint32_t idxCount;   /* IdxBuffer.Size */
    uint32_t firstCmd;   /* the list's commands are cmds[firstCmd .. firstCmd + cmdCount) */
    uint32_t cmdCount;
} SailorUiDrawList;
/* ImGui_SetupRenderState's push constants (:118-125) and ImGui_RenderDrawData's loop (:197-275) in fp32: width = (int)(displaySize.x * framebufferScale.x),
 * height likewise; *outNumCommands = 0 when either is <= 0.  Otherwise outPushConstants = scale.x, scale.y, translate.x, translate.y and, per command that
 * is no callback and survives `clipMax <= clipMin` after the clamps, one SailorUiCommand with the global offsets and the scissor of :250-251.  At most
 * maxCommands are written (outCommands may be NULL to count); *outNumCommands is the number there are.  outWidth / outHeight (may be NULL) get width, height. */
SAILOR_HIP_API int sailor_host_ui_flatten(const float displayPos[2], const float displaySize[2], const float framebufferScale[2], const SailorUiDrawList* lists,
                                          uint32_t numLists, const SailorUiDrawCmd* cmds, uint32_t numCmds, float outPushConstants[4], SailorUiCommand* outCommands,
                                          uint32_t maxCommands, uint32_t* outNumCommands, int32_t* outWidth, int32_t* outHeight);

/* ---- ExperimentalParticles: update, shadow map, lit draw (particles.hip) ---------------------------------------------------------------------------
 * Replaces: FrameGraph/ParticlesNode.cpp:184-257 -- the Dispatch of Content/Experimental/MeshParticles/ComputeParticles.shader:85-137 on the transfer
 * list, the node-owned R32_SFLOAT shadow map drawn with Particle.shader under SHADOW_CASTER (ParticleShadow.mat), and the colour pass of Particle.shader
 * (Particle.mat) into Main / DepthBuffer.
 * Pinned:
 *  1. Update.  frame = uint(mod(currentTime * float(fps), float(numFrames))), current = uint(mod(float(instanceId), float(traceFrames))) (GLSL's mod takes
 *     floats: the uints are converted, as written at :100-101), mod(x, y) = x - y * floor(x / y), decay = pow(traceDecay, float(current)).  uint(f) is
 *     the device's saturating conversion (NaN and negatives -> 0).  The two record indices (:106-107) are
 *       (frame - current [- 1]) * numInstances / traceFrames + instanceId / traceFrames
 *     in 32-bit UNSIGNED arithmetic that wraps.  `max(0, uintExpr)`: GLSL has max(int, int) and max(uint, uint) but no mixed form; the literal 0 is an int
 *     and converts implicitly to uint (int -> uint is an implicit conversion, uint -> int is not), so the call resolves to max(uint, uint) and clamps
 *     nothing.  A record index >= numRecords reads an ALL-ZERO record (what robust buffer access gives an SSBO load); the kernel never reads outside the
 *     buffer.  So while frame < current + 1 -- the first frames of a loop -- a trail instance gets the zero record.
 *  2. model = translate((p1 + p2) * 0.5) * rotation * scale, the two products as full 4 x 4 GLSL products (column j = ((c0 b0j + c1 b1j) + c2 b2j) + c3 b3j).
 *     rotation = rotationMatrix(cross(up, dir), acos(dot(up, dir))) (:60-82) with up = (0, 0, 1), dir = normalize(p2 - p1), applied only if
 *     length(axis) > 0, else the identity; scale = diag(s, s, distance(p2, p1), 1), s = size2 * decay * 1.5.  dot = (xx + yy) + zz, IEEE division and
 *     square root, normalize(v) = v / sqrt(dot(v, v)); sinf, cosf, acosf, powf are the device library's.  Kept, not repaired: dir == +-up gives the
 *     identity (-up is not flipped); p1 == p2 gives a NaN direction, a NaN axis, a false compare, the identity and a zz scale of 0; a zero record gives
 *     an all-zero scale, so the instance draws nothing.
 *  3. colorOld = (rgb2, a2 * decay) of the old record, color the same of the new one, isCulled = enabled > 0.5 ? 1 : 0 (no shader reads it).
 *     materialInstance and the 8 bytes of padding are NOT written.
 *  4. Shadow map.  The only attachment, no depth test: the LAST primitive in primitive order that covers a texel owns it, whatever its depth.
 *     clip = (lightsMatrices[0] * model) * vec4(p, 1) (Particle.shader:125, GLSL's left-to-right product), then the rules of sailor_hip_raster_depth:
 *     near-plane cut, flipped viewport, 1/256-texel snapping, 64-bit edge functions, top-left rule, cull Back, z by the raster formula, fragments outside
 *     (0, 1] do not exist.  order = (instance * numTriangles + triangle) * 2 + part.  A key per texel, (order + 1) << 32 | depthBits, under an unsigned
 *     maximum; a store pass writes the low word, an untouched texel is 0 (the clear value).
 *  5. Colour pass.  Depth test and write against DepthBuffer, GreaterOrEqual in primitive order: the surface pass's key, depthBits << 32 | (order + 1),
 *     seeded from the depth buffer; clip = projection * (view * (model * p)).  Varyings at the winning fragment by the surface pass's formula:
 *     worldPosition = (model * p).xyz / w, color = color * (1 - a) + colorOld * a with a = (p.z + 1) / 2 (mix, :130), N = mat3(model) * inNormal
 *     (tangentBasis * (0, 0, 1) is its third column: the first two meet zeros).  Fragment (:246-252): n = normalize(N), lighting = max(0, dot(-light[0].direction, n)),
 *     shadow = ShadowCalculation_Pcf(map, lightsMatrices[0] * vec4(worldPosition, 1), 0.00001) (Lighting.glsl:242-261, :168-196: divide by w, all three
 *     coordinates * 0.5 + 0.5, y flipped, 1 outside [0, 1]^2 or for z < 0.5, sixteen bilinear Clamp taps `.r * 0.5 + 0.5`, currentDepth + bias > pcfDepth),
 *     rgb = color.rgb * max(0.05, min(lighting, shadow)), alpha the interpolated colour's.  Where a particle primitive owns the pixel, Main (RGBA32F) and
 *     DepthBuffer are written; everything else in both is left as it was.
 * Light record 0 and matrix 0 are read on the device.  All entry points record only (no allocation, no read-back, no wait: capturable); a refused call
 * launches nothing, returns SAILOR_HIP_ERR_INVALID_ARGUMENT and leaves its text in last_error. */

/* ParticlesNode.h:44-51 ParticleData == ComputeParticles.shader:20-27.  80 bytes. */
typedef struct SailorParticleData {
    float enabled, size1, size2, _nouse; /*  0 */
    float xyz1[3], _w1;                  /* 16 */
    float rgba1[4];                      /* 32 */
    float xyz2[3], _w2;                  /* 48 */
    float rgba2[4];                      /* 64 */
} SailorParticleData;

/* ParticlesNode.h:62-71 PerInstanceData == Particle.shader:34-41, std430.  112 bytes. */
typedef struct SailorParticleInstance {
    float model[16];            /*   0 */
    float color[4];             /*  64 */
    float colorOld[4];          /*  80 */
    uint32_t materialInstance;  /*  96 */
    uint32_t isCulled;          /* 100 */
    uint32_t _pad[2];           /* 104 */
} SailorParticleInstance;

/* ParticlesNode.h:53-60 PushConstants == ComputeParticles.shader:51-58.  20 bytes. */
typedef struct SailorParticlesConstants {
    uint32_t numInstances; /*  0 */
    uint32_t numFrames;    /*  4 */
    uint32_t fps;          /*  8 */
    uint32_t traceFrames;  /* 12 */
    float traceDecay;      /* 16 */
} SailorParticlesConstants;

/* the particle mesh (BindVertexBuffer / BindIndexBuffer / DrawIndexed of ParticlesNode.cpp:223-225, :254-256), drawn numInstances times */
typedef struct SailorParticlesDraw {
    const SailorVertexP3N3T3B3UV2C4* dVertices; /* device, already offset by vertexOffset */
    const uint32_t* dIndices;                   /* device, 3 x numTriangles, already offset by firstIndex */
    uint32_t numTriangles;
    uint32_t _pad;
} SailorParticlesDraw;

/* Replaces: Dispatch(256, 1, 1) of ComputeParticles.shader (ParticlesNode.cpp:192): k_particles_update, a lane per instance (the shader's 256-thread
 * partition is not observable).  frame: currentTime is read.  dRecords: device, numRecords records (16-byte aligned); dInstances: device,
 * constants->numInstances instances.  Refused: NULL / misaligned pointers, overlapping buffers, numInstances, traceFrames or numFrames == 0, numInstances above 2^31 - 1,
 * traceDecay not finite or not > 0, currentTime * fps not finite or negative. */
SAILOR_HIP_API int sailor_hip_particles_update(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorParticlesConstants* constants,
                                               const SailorParticleData* dRecords, uint32_t numRecords, SailorParticleInstance* dInstances);
/* the workspace both passes use, one after the other: a 64-bit key per texel of the larger of the map and the frame; 0 = invalid extents */
SAILOR_HIP_API size_t sailor_hip_particles_workspace_bytes(int32_t mapWidth, int32_t mapHeight, int32_t width, int32_t height);
/* Replaces: the shadow pass of ParticlesNode.cpp:196-229: k_particles_seed (keys = 0), k_particles_cast, k_particles_store_map.
 *   dLightsMatrices : device, matrix 0 is read       dShadowMap : device out, mapWidth x mapHeight floats, every texel written
 * Refused besides the above: a map that overlaps the instances or the workspace, numInstances == 0, numTriangles == 0, extents outside 1 .. 32768,
 * numInstances * 2 * numTriangles reaching 2^32 - 1, a workspace smaller than 8 * mapWidth * mapHeight bytes. */
SAILOR_HIP_API int sailor_hip_particles_shadow(SailorHipContext* ctx, const SailorParticlesDraw* draw, const SailorParticleInstance* dInstances, uint32_t numInstances,
                                               const float* dLightsMatrices, float* dShadowMap, int32_t mapWidth, int32_t mapHeight, void* dWorkspace,
                                               size_t workspaceBytes);
/* Replaces: the colour pass of ParticlesNode.cpp:232-257: k_particles_seed (keys = depth bits << 32), k_particles_visibility, k_particles_resolve.
 *   frame : view and projection are read      dLights : device, record 0 is read      dShadowMap : device, what sailor_hip_particles_shadow wrote
 *   dMain : device in / out, width x height float4       dDepth : device in / out, width x height floats
 * Refused as above, with dMain / dDepth against the map, the instances and the workspace, and a workspace smaller than 8 * width * height bytes. */
SAILOR_HIP_API int sailor_hip_particles_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorParticlesDraw* draw,
                                             const SailorParticleInstance* dInstances, uint32_t numInstances, const SailorLightShaderData* dLights,
                                             const float* dLightsMatrices, const float* dShadowMap, int32_t mapWidth, int32_t mapHeight, float* dMain,
                                             float* dDepth, int32_t width, int32_t height, void* dWorkspace, size_t workspaceBytes);

#ifdef __cplusplus
}
#endif
#endif /* SAILOR_HIP_H */
