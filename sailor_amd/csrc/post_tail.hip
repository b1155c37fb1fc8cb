// The tail of the shipped frame graph for gfx950 (tests/golden/DefaultRenderer.renderer:322-353): the two PostProcess draws that end the frame.
//
// Replaces the GPU work of
//   * PostProcess with Content/Shaders/MotionBlur.shader:63-102 (reads Secondary and DepthBuffer, writes Main)                    -> k_motion_blur
//   * PostProcess with Content/Shaders/Debug.shader:115-178 under no define or one of AO, LIGHT_TILES, CASCADES (writes BackBuffer) -> k_debug_view<MODE>
// Colour images are RGBA32F, 16-byte aligned; depth, linear depth and g_AO are single-channel fp32 planes; row 0 = top; texel (i, j) of a w x h
// target has fragTexcoord = ((i + 0.5) / w, (j + 0.5) / h) and gl_FragCoord = (i + 0.5, j + 0.5).
//
// Arithmetic is evaluated exactly as the shaders write it, in their order, one IEEE rounding per operation (-ffp-contract=off, IEEE division and
// square root, denormals kept), with the evaluation orders hbao.hip fixes: mat4 * vec4 row by row left to right (glsl_mul), v / s = one division per
// component, length = sqrt(dot), dot(a, b) of two-vectors = a.x b.x + a.y b.y, mix(a, b, t) = a (1 - t) + b t.  tests/tail_ref.py restates it in
// NumPy float32 and the kernels reproduce it bit for bit.
//
// Decisions where "as written" needs one (MotionBlur.shader line numbers):
//   * inverse(frame.projection) (:69), inverse(frame.view) (:72) and previousFrame.projection * previousFrame.view (:74) are uniform per draw: the entry
//     point computes them once on the host with host_math.cpp's inverse / mul (glm's order, what sailor_host_mat4_inverse / _mul export) and passes them
//     by value.  frame.invProjection is NOT used: the shader writes the literal inverse().
//   * min, max and clamp(x, 0, 1) are the GLSL definitions of common.h, so min(1, NaN) = 1 (:81-82).  On the first frame previousFrame is all
//     zeros (RHIFrameGraph.cpp:189: m_prevFrameData is value-initialised), previousClipPos is 0 / 0 everywhere and the velocity is (intensity, intensity).
//   * no lower clamp on the velocity (:81-82 clamp above only): a large negative velocity piles the taps up on the 0 edge.
//   * clamp(x, 0, 1) (:95) passes a NaN through; the early-out is length(velocity) <= 0.0001 (:87) -- a NaN length fails it and blurs.
//   * int(data.samples) truncates, the loop runs int(samples) - 1 taps (:93), the division is by float(data.samples) itself (:100).  Alpha is 1.
//   * depthSampler / colorSampler: bilinear, clamp-to-edge, the taps and weights of sampling.h evaluated per fetch, with the saturating float -> int
//     conversion (NaN -> 0) its header documents for non-finite coordinates (bilinear_taps_saturating).
// Debug.shader line numbers:
//   * no define: texture(ldrSceneSampler, uv) (:117).  AO (:120): the one-channel g_aoSampler, bilinear, broadcast to four channels.
//   * LIGHT_TILES (:122-144), literal: screenUv.y = viewportSize.y - gl_FragCoord.y, tileId = ivec2(screenUv) / 16, numTiles = floor(viewportSize / 16)
//     with the mod / padding term, tileIndex = uint(tileId.y * (numTiles.x + padding.x) + tileId.x) in float, the sentinel break at 0xFFFFFFFF, and
//     0.05 added ONCE PER LISTED LIGHT as sequential fp32 additions onto linearDepth / 50000 (not n * 0.05: the base differs per pixel).
//     linearDepthSampler is Nearest (DefaultRenderer.renderer:85-90): nearest_clamp.  The target must have the frame's extent (gl_FragCoord indexes the
//     frame's tiles); a list entry past the reference's capacity of the culledLights buffer (tiles * 128 + 1 words, LightCullingNode.cpp:64) ends the
//     list like the sentinel does, so that a damaged grid cannot send a read outside the buffer.
//   * CASCADES (:146-173): the first i with linearDepth < cameraZNearZFar.y * ShadowCascadeLevels[i], else NUM_CSM_CASCADES; layers 3 and 4 share the
//     else colour (the initial (1, 0, 0) of :157 is dead); rgb = mix(rgb, dColor, 0.5), alpha passes through.
//
// Shape.  One texel per lane, 256-thread blocks of 64 x 4 texels, no LDS, no barrier, colour moved as 16-byte loads and stores; the frame constants
// are kernel arguments (scalar registers).  Both passes are memory-bound: motion blur reads 4 depth taps and 4 x int(samples) colour taps per texel
// from planes that neighbouring lanes share, the debug view one to four texels.  LIGHT_TILES counts its tile's list in the lane: the 16 lanes of a
// tile row read the same addresses (one request per distinct address), a wave covers four tiles, and a list is at most 128 words -- against a per-tile
// count pass, which would add a launch, a workspace and a dependency for 0.4 % of the frame's texels' worth of reads.  Not measured against it.
#include "common.h"
#include "sampling.h"
#include "texel_pass.h"
#include <math.h>

// ---- a. motion blur -----------------------------------------------------------------------------------------------------------------------
struct MotionBlurArgs {
    Mat4 invProjection;    // inverse(frame.projection)
    Mat4 invView;          // inverse(frame.view)
    Mat4 prevViewProjection; // previousFrame.projection * previousFrame.view
    SailorMotionBlurParams p;
};

__global__ __launch_bounds__(256) void k_motion_blur(const float* __restrict__ depth, int DW, int DH, const float4* __restrict__ color, int CW, int CH,
                                                     float4* __restrict__ dst, int W, int H, const MotionBlurArgs A)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    float4* __restrict__ out = dst + (size_t)j * (size_t)W + i;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;

    const float d = sample_clamp_f1(depth, DW, DH, u, v); // :65
    const float ndcX = u * 2.0f - 1.0f, ndcY = v * 2.0f - 1.0f; // :66
    float4 viewPos = glsl_mul(A.invProjection, ndcX, ndcY, d, 1.0f); // :69
    const float vw = viewPos.w;
    viewPos.x = viewPos.x / vw; viewPos.y = viewPos.y / vw; viewPos.z = viewPos.z / vw; viewPos.w = viewPos.w / vw; // :70
    const float4 worldPos = glsl_mul(A.invView, viewPos.x, viewPos.y, viewPos.z, viewPos.w);                        // :72
    const float4 prevClip = glsl_mul(A.prevViewProjection, worldPos.x, worldPos.y, worldPos.z, worldPos.w);          // :74
    const float prevX = prevClip.x / prevClip.w, prevY = prevClip.y / prevClip.w;                                    // :75
    float velX = (ndcX - prevX) / 2.0f, velY = (ndcY - prevY) / 2.0f; // :77
    velX = velX / A.p.maxSpeed; velY = velY / A.p.maxSpeed;           // :79
    velX = glsl_min(1.0f, velX) * A.p.intensity;                      // :81
    velY = glsl_min(1.0f, velY) * A.p.intensity;                      // :82

    const float4 c0 = sample_clamp_f4_saturating(color, CW, CH, u, v); // :84
    float r = c0.x, g = c0.y, b = c0.z;
    if (sqrtf(velX * velX + velY * velY) <= 0.0001f) { *out = make_float4(r, g, b, 1.0f); return; } // :87-91

    float tu = u, tv = v;
    const int n = (int)A.p.samples; // the entry point keeps samples within [1, 64]
    for (int k = 1; k < n; k++) {   // :93-98
        tu = glsl_saturate(tu + velX); tv = glsl_saturate(tv + velY);
        const float4 c = sample_clamp_f4_saturating(color, CW, CH, tu, tv);
        r = r + c.x; g = g + c.y; b = b + c.z;
    }
    *out = make_float4(r / A.p.samples, g / A.p.samples, b / A.p.samples, 1.0f); // :100-101
}

// ---- b. the debug view ----------------------------------------------------------------------------------------------------------------------
struct DebugViewArgs {
    int viewportW, viewportH; // frame.viewportSize
    float zFar;               // frame.cameraZNearZFar.y
    uint32_t culledCapacity;  // words of the reference's culledLights buffer for this viewport
};

__constant__ float c_shadowCascadeLevels[SAILOR_NUM_CSM_CASCADES] = SAILOR_SHADOW_CASCADE_LEVELS;

template <int MODE>
__global__ __launch_bounds__(256) void k_debug_view(const float4* __restrict__ scene, int SW, int SH, const float* __restrict__ linearDepth, int DW, int DH,
                                                    const SailorLightsGrid* __restrict__ grid, const uint32_t* __restrict__ culled, const float* __restrict__ ao,
                                                    int AW, int AH, float4* __restrict__ dst, int W, int H, const DebugViewArgs A)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    float4* __restrict__ out = dst + (size_t)j * (size_t)W + i;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;

    if (MODE == SAILOR_DEBUG_VIEW_SCENE) { *out = sample_clamp_f4_saturating(scene, SW, SH, u, v); return; } // :117
    if (MODE == SAILOR_DEBUG_VIEW_AO) { // :120
        const float a = sample_clamp_f1(ao, AW, AH, u, v);
        *out = make_float4(a, a, a, a);
        return;
    }
    const float ld = linearDepth[(size_t)nearest_clamp(DH, v) * (size_t)DW + nearest_clamp(DW, u)];
    if (MODE == SAILOR_DEBUG_VIEW_LIGHT_TILES) {
        const float base = ld / 50000.0f; // :122
        const float numTilesX = floorf((float)A.viewportW / (float)TILE); // :124 (.y is not read)
        const float screenX = (float)i + 0.5f, screenY = (float)A.viewportH - ((float)j + 0.5f); // :125
        const int tileX = (int)screenX / TILE, tileY = (int)screenY / TILE;                      // :126
        const int padX = min(1, A.viewportW % TILE);                                             // :128-129
        const uint32_t tileIndex = (uint32_t)((float)tileY * (numTilesX + (float)padX) + (float)tileX); // :131
        const SailorLightsGrid cell = grid[tileIndex];                                                  // :133-134
        float c = base;
        for (uint32_t k = 0; k < cell.num; k++) { // :136-144
            const uint64_t at = (uint64_t)cell.offset + k;
            if (at >= A.culledCapacity) break; // (outside the reference's buffer: header)
            if (culled[at] == 0xFFFFFFFFu) break;
            c = c + 0.05f;
        }
        *out = make_float4(c, c, c, base);
        return;
    }
    // CASCADES (:146-173)
    float4 o = sample_clamp_f4_saturating(scene, SW, SH, u, v);
    int layer = SAILOR_NUM_CSM_CASCADES;
#pragma unroll
    for (int k = SAILOR_NUM_CSM_CASCADES - 1; k >= 0; k--) // the first k that passes = the lowest one
        if (ld < A.zFar * c_shadowCascadeLevels[k]) layer = k;
    const float dr = layer == 1 ? 1.0f : 0.0f, dg = layer == 2 ? 0.0f : 1.0f, db = (layer == 0 || layer == 1) ? 0.0f : 1.0f; // :157-171
    o.x = o.x * (1.0f - 0.5f) + dr * 0.5f; o.y = o.y * (1.0f - 0.5f) + dg * 0.5f; o.z = o.z * (1.0f - 0.5f) + db * 0.5f; // :173
    *out = o;
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
#define TAIL_MAX_SAMPLES 64.0f

extern "C" {

int sailor_hip_motion_blur(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorUboFrameData* previousFrame, const float* dDepth, int32_t depthWidth,
                           int32_t depthHeight, const float* dColor, int32_t colorWidth, int32_t colorHeight, const SailorMotionBlurParams* params, float* dOut,
                           int32_t width, int32_t height)
{
    if (!ctx || !frame || !previousFrame || !params || !aligned(dDepth, 4) || !aligned(dColor, 16) || !aligned(dOut, 16) || !extent_ok(depthWidth, depthHeight) ||
        !extent_ok(colorWidth, colorHeight) || !extent_ok(width, height))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    // the loop count is int(samples): a NaN, an infinity or anything outside [1, 64] is refused rather than run without an end; 1 / maxSpeed = 0 has no velocity
    if (!(params->samples >= 1.0f && params->samples <= TAIL_MAX_SAMPLES) || params->maxSpeed == 0.0f) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (overlaps(dOut, (size_t)width * height * 16, dColor, (size_t)colorWidth * colorHeight * 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT; // taps read what other lanes write
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    MotionBlurArgs A;
    sailor_host_mat4_inverse(frame->projection, A.invProjection.m);
    sailor_host_mat4_inverse(frame->view, A.invView.m);
    sailor_host_mat4_mul(previousFrame->projection, previousFrame->view, A.prevViewProjection.m);
    A.p = *params;
    sailor_launch(ctx, k_motion_blur, texel_grid(width, height), dim3(256), dDepth, (int)depthWidth, (int)depthHeight, (const float4*)dColor, (int)colorWidth,
                  (int)colorHeight, (float4*)dOut, (int)width, (int)height, A);
    SAILOR_CHECK_LAUNCH(ctx, "k_motion_blur");
    return SAILOR_HIP_OK;
}

int sailor_hip_debug_view(SailorHipContext* ctx, const SailorUboFrameData* frame, int32_t mode, const float* dLdrScene, int32_t sceneWidth, int32_t sceneHeight,
                          const float* dLinearDepth, int32_t depthWidth, int32_t depthHeight, const SailorLightsGrid* dLightsGrid, const uint32_t* dCulledLights,
                          const float* dAo, int32_t aoWidth, int32_t aoHeight, float* dOut, int32_t width, int32_t height)
{
    if (!ctx || !frame || !aligned(dOut, 16) || !extent_ok(width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const bool needScene = mode == SAILOR_DEBUG_VIEW_SCENE || mode == SAILOR_DEBUG_VIEW_CASCADES;
    const bool needDepth = mode == SAILOR_DEBUG_VIEW_LIGHT_TILES || mode == SAILOR_DEBUG_VIEW_CASCADES;
    if (mode < SAILOR_DEBUG_VIEW_SCENE || mode > SAILOR_DEBUG_VIEW_CASCADES) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (needScene && (!aligned(dLdrScene, 16) || !extent_ok(sceneWidth, sceneHeight) || overlaps(dOut, (size_t)width * height * 16, dLdrScene, (size_t)sceneWidth * sceneHeight * 16)))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (needDepth && (!aligned(dLinearDepth, 4) || !extent_ok(depthWidth, depthHeight))) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (mode == SAILOR_DEBUG_VIEW_AO && (!aligned(dAo, 4) || !extent_ok(aoWidth, aoHeight))) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    DebugViewArgs A {};
    A.viewportW = frame->viewportSize[0]; A.viewportH = frame->viewportSize[1];
    A.zFar = frame->cameraZNearZFar[1];
    if (mode == SAILOR_DEBUG_VIEW_LIGHT_TILES) {
        // gl_FragCoord indexes the frame's tiles: on a target of another extent the shader's tile index leaves the grid
        if (!aligned(dLightsGrid, 4) || !aligned(dCulledLights, 4) || width != A.viewportW || height != A.viewportH) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
        int32_t tx = 0, ty = 0;
        if (sailor_hip_num_tiles(width, height, &tx, &ty) != SAILOR_HIP_OK) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
        A.culledCapacity = (uint32_t)((size_t)tx * ty * KEEP + 1);
    }
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid = texel_grid(width, height), block(256);
#define TAIL_LAUNCH(M)                                                                                                                                         \
    sailor_launch(ctx, k_debug_view<M>, grid, block, (const float4*)dLdrScene, (int)sceneWidth, (int)sceneHeight, dLinearDepth, (int)depthWidth, (int)depthHeight, \
                  dLightsGrid, dCulledLights, dAo, (int)aoWidth, (int)aoHeight, (float4*)dOut, (int)width, (int)height, A)
    switch (mode) {
    case SAILOR_DEBUG_VIEW_SCENE: TAIL_LAUNCH(SAILOR_DEBUG_VIEW_SCENE); break;
    case SAILOR_DEBUG_VIEW_AO: TAIL_LAUNCH(SAILOR_DEBUG_VIEW_AO); break;
    case SAILOR_DEBUG_VIEW_LIGHT_TILES: TAIL_LAUNCH(SAILOR_DEBUG_VIEW_LIGHT_TILES); break;
    default: TAIL_LAUNCH(SAILOR_DEBUG_VIEW_CASCADES); break;
    }
#undef TAIL_LAUNCH
    SAILOR_CHECK_LAUNCH(ctx, "k_debug_view");
    return SAILOR_HIP_OK;
}

} // extern "C"
