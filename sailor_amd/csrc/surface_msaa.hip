// The multisampled RenderScene pass: per-sample visibility keys, shaded layers, the AVERAGE resolve.  The rules are pinned in include/sailor_hip.h (the
// Multisampled section); tests/msaa_ref.py restates them sample by sample and the kernels are held to it bit for bit.  The pattern is the Transparent bucket
// route's: the draws run once and keep several keys a pixel; every layer is then read out into an ordinary surface workspace and goes through the unchanged
// resolve and shade; here the layers are weighted by the samples they own and summed.
//
//   k_surface_msaa, k_surface_msaa_gltf  surface_masked_body.h's draw with SURF_DRAW_MSAA: the set-up and the alpha helpers of the Masked queue, the walk of
//                                        surface_fill_msaa.h over pixels, surf_pixel_msaa per pixel -- a relaxed load per covered sample, the discard once
//                                        a pixel at its centre and only if a sample would win, a 64-bit atomicMax per winning sample.  The store is
//                                        pixel-major, store[(row * W + x) * S + s]: a fragment touches one run of S x 8 bytes.
//   k_surface_msaa_begin                 a lane per key: sampleDepthBits << 32, or 0.
//   k_surface_msaa_layer                 a lane per pixel of 8 rows: the pixel's S keys by 16-byte loads, its (k + 1)-th smallest distinct order as an
//                                        ordinary workspace key, the weight byte, the uncovered byte (k = 0), the clipped samples folded into the last
//                                        layer; the two counters are summed per wave (ballot, popcount) and added by one lane.  Stateless: no per-pixel cursor.
//   k_surface_msaa_accumulate            a lane per pixel: target = (u / S) target + (w0 / S) c0, then += (wk / S) ck; every product and sum rounded on its own.
//   k_surface_msaa_store_depth           a lane per pixel: the S sample depths for the next pass's begin, and their AVERAGE into the depth attachment.
#include "surface_masked_body.h"

#define MSAA_MAX_SAMPLES 8

__global__ __launch_bounds__(256) void k_surface_msaa(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                      const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                      const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H, int rowBegin,
                                                      int rows, void* __restrict__ workspace, unsigned long long* __restrict__ store, int samples, unsigned long long pattern)
{
    SurfMsaa x;
    x.store = store; x.pattern = pattern; x.samples = samples;
    surf_visibility_masked<false, false, SURF_DRAW_MSAA>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace, x);
}

__global__ __launch_bounds__(256) void k_surface_msaa_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                           const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                           const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                           int rowBegin, int rows, void* __restrict__ workspace, unsigned long long* __restrict__ store, int samples,
                                                           unsigned long long pattern)
{
    SurfMsaa x;
    x.store = store; x.pattern = pattern; x.samples = samples;
    surf_visibility_masked<true, false, SURF_DRAW_MSAA>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace, x);
}

__global__ __launch_bounds__(256) void k_surface_msaa_begin(unsigned long long* __restrict__ store, const uint32_t* __restrict__ sampleDepth, size_t keys)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < keys) store[g] = sampleDepth ? (unsigned long long)sampleDepth[g] << 32 : 0ull;
}

// the S keys of a pixel as orders and depth words, by 16-byte loads (the store is 16-byte aligned and S x 8 bytes a pixel); a slot beyond S: order 0, depth 0
__device__ __forceinline__ void msaa_load_pixel(const unsigned long long* __restrict__ p, int S, bool inside, uint32_t (&o)[MSAA_MAX_SAMPLES], uint32_t (&zb)[MSAA_MAX_SAMPLES])
{
#pragma unroll
    for (int s = 0; s < MSAA_MAX_SAMPLES; s++) { o[s] = 0; zb[s] = 0; }
    if (!inside) return;
    if (S == 1) {
        const unsigned long long v = p[0];
        o[0] = (uint32_t)v; zb[0] = (uint32_t)(v >> 32);
        return;
    }
#pragma unroll
    for (int s = 0; s < MSAA_MAX_SAMPLES; s += 2)
        if (s < S) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p + s);
            o[s] = (uint32_t)v.x; zb[s] = (uint32_t)(v.x >> 32); o[s + 1] = (uint32_t)v.y; zb[s + 1] = (uint32_t)(v.y >> 32);
        }
}

// k_surface_bucket_layer's shape: a wave adds what it found in 64 pixels of 8 rows ONCE.  (No lane leaves before the ballots.)
#define MSAA_LAYER_ROWS 8
__global__ __launch_bounds__(256) void k_surface_msaa_layer(void* __restrict__ workspace, const unsigned long long* __restrict__ store, int S, uint32_t layers, uint32_t k,
                                                            uint8_t* __restrict__ weight, uint8_t* __restrict__ uncovered, uint32_t* __restrict__ count,
                                                            uint32_t* __restrict__ clipped, int W, int rows)
{
    const int i = texel_i(), j0 = texel_j() * MSAA_LAYER_ROWS;
    const SurfWorkspace ws = surf_workspace(workspace, (size_t)rows * W);
    uint32_t found = 0, cut = 0;
    for (int r = 0; r < MSAA_LAYER_ROWS; r++) {
        const int jb = j0 + r;
        const size_t at = (size_t)jb * W + i;
        const bool inside = i < W && jb < rows;
        uint32_t o[MSAA_MAX_SAMPLES], zb[MSAA_MAX_SAMPLES];
        msaa_load_pixel(store + at * (size_t)S, S, inside, o, zb);
        // the (k + 1)-th smallest distinct non-zero order (an order never reaches 2^32 - 1: the draw entries refuse it)
        uint32_t cur = 0;
#pragma unroll 1
        for (uint32_t t = 0; t <= k; t++) {
            uint32_t next = 0xFFFFFFFFu;
#pragma unroll
            for (int s = 0; s < MSAA_MAX_SAMPLES; s++) next = (o[s] > cur && o[s] < next) ? o[s] : next;
            cur = next == 0xFFFFFFFFu ? 0u : next;
            if (!cur) break;
        }
        uint32_t w = 0, z = 0, beyond = 0, none = 0;
#pragma unroll
        for (int s = MSAA_MAX_SAMPLES - 1; s >= 0; s--) {
            if (cur && o[s] == cur) { w++; z = zb[s]; } // (downwards: z ends as the lowest-numbered sample's)
            beyond += (cur && o[s] > cur) ? 1u : 0u;
            none += (s < S && o[s] == 0u) ? 1u : 0u;
        }
        const bool clips = k + 1u == layers && beyond != 0u; // (with layers == S a pixel has no order beyond its S-th)
        if (clips) w += beyond;
        if (inside) {
            ws.keys[at] = cur ? ((unsigned long long)z << 32) | cur : 0ull;
            weight[at] = (uint8_t)w;
            if (k == 0) uncovered[at] = (uint8_t)none;
        }
        found += (uint32_t)__popcll(__ballot(cur != 0u));
        cut += (uint32_t)__popcll(__ballot(clips));
    }
    if ((threadIdx.x & 63) == 0) {
        if (found) atomicAdd(count, found);
        if (cut && clipped) atomicAdd(clipped, cut);
    }
}

// rule 9: terms of weight 0 are omitted, not multiplied; w0 == S stores c0's bits.  (-ffp-contract=off: no product is fused into a sum.)
__global__ __launch_bounds__(256) void k_surface_msaa_accumulate(const float4* __restrict__ radiance, const float4* __restrict__ emissive, const uint8_t* __restrict__ weight,
                                                                 const uint8_t* __restrict__ uncovered, int S, uint32_t k, float4* __restrict__ target, int W, int rows)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const size_t at = (size_t)jb * W + i;
    const int w = weight[at];
    if (w == 0) return;
    float4 c = radiance[at];
    if (emissive) {
        const float4 e = emissive[at];
        c = make_float4(e.x + c.x, e.y + c.y, e.z + c.z, c.w); // k_surface_composite_gltf's sum
    }
    if (k == 0 && w == S) { target[at] = c; return; }
    const float f = (float)w / (float)S; // exact: S is a power of two
    const float4 a = make_float4(f * c.x, f * c.y, f * c.z, f * c.w);
    if (k == 0) {
        const int u = uncovered[at];
        if (u == 0) { target[at] = a; return; }
        const float g = (float)u / (float)S;
        const float4 t = target[at];
        target[at] = make_float4(g * t.x + a.x, g * t.y + a.y, g * t.z + a.z, g * t.w + a.w);
        return;
    }
    const float4 t = target[at];
    target[at] = make_float4(t.x + a.x, t.y + a.y, t.z + a.z, t.w + a.w);
}

__global__ __launch_bounds__(256) void k_surface_msaa_store_depth(const unsigned long long* __restrict__ store, int S, float* __restrict__ sampleDepth, float* __restrict__ depth,
                                                                  int W, int rowBegin, int rows)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const size_t at = (size_t)jb * W + i;
    uint32_t o[MSAA_MAX_SAMPLES], zb[MSAA_MAX_SAMPLES];
    msaa_load_pixel(store + at * (size_t)S, S, true, o, zb);
    float sum = __uint_as_float(zb[0]);
#pragma unroll
    for (int s = 1; s < MSAA_MAX_SAMPLES; s++)
        if (s < S) sum = sum + __uint_as_float(zb[s]);
    if (sampleDepth) {
#pragma unroll
        for (int s = 0; s < MSAA_MAX_SAMPLES; s++)
            if (s < S) sampleDepth[at * (size_t)S + s] = __uint_as_float(zb[s]);
    }
    if (depth) depth[(size_t)(rowBegin + jb) * W + i] = sum * (1.0f / (float)S);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
// Vulkan's standard sample locations (VkPhysicalDeviceLimits::standardSampleLocations), in 1/256 pixel from the pixel's top-left corner
static const int32_t* msaa_table(uint32_t samples)
{
    static const int32_t t1[] = {128, 128};
    static const int32_t t2[] = {192, 192, 64, 64};
    static const int32_t t4[] = {96, 32, 224, 96, 32, 160, 160, 224};
    static const int32_t t8[] = {144, 80, 112, 176, 208, 144, 80, 48, 48, 208, 16, 112, 176, 240, 240, 16};
    return samples == 1u ? t1 : samples == 2u ? t2 : samples == 4u ? t4 : samples == 8u ? t8 : nullptr;
}
// the table as the kernels take it: byte s = (sy / 16) << 4 | (sx / 16) (surface_fill_msaa.h)
static unsigned long long msaa_pattern(uint32_t samples)
{
    const int32_t* t = msaa_table(samples);
    unsigned long long p = 0;
    for (uint32_t s = 0; s < samples; s++) p |= (unsigned long long)(((t[2 * s + 1] / 16) << 4) | (t[2 * s] / 16)) << (8 * s);
    return p;
}
static bool msaa_extent_ok(int32_t width, const SailorBand* band)
{
    return band && width > 0 && width <= TEXEL_MAX_EXTENT && band->fbRowCount > 0 && band->fbRowCount <= TEXEL_MAX_EXTENT;
}

// what every entry checks of the store: why not, or NULL.  (The band has been checked by then.)
static const char* msaa_store_why(int32_t width, const SailorBand* band, const void* dStore, size_t storeBytes, uint32_t samples)
{
    if (!msaa_table(samples)) return "samples is not 1, 2, 4 or 8";
    if (!aligned(dStore, 16)) return "the sample store is NULL or not 16-byte aligned";
    if (storeBytes < sailor_hip_surface_msaa_bytes(width, band, samples)) return "the sample store is smaller than sailor_hip_surface_msaa_bytes";
    return nullptr;
}
static int msaa_draw_refusals(SailorHipContext* ctx, const char* who, int32_t width, const SailorBand* band, const void* dStore, size_t storeBytes, uint32_t samples)
{
    if (const char* why = msaa_store_why(width, band, dStore, storeBytes, samples)) return surf_refuse(ctx, who, why);
    return SAILOR_HIP_OK;
}
// the weight and uncovered planes of _msaa_layer and _msaa_accumulate
static const char* msaa_planes_why(uint32_t samples, uint32_t layers, uint32_t k, const uint8_t* dWeight, const uint8_t* dUncoveredOrNull)
{
    if (layers < 1u || layers > samples) return "layers is outside 1 .. samples";
    if (k >= layers) return "k is not below layers";
    if (!dWeight) return "the weight plane is NULL";
    if (k == 0u && !dUncoveredOrNull) return "layer 0 needs the uncovered plane";
    return nullptr;
}

extern "C" {

int sailor_host_msaa_sample_positions(uint32_t samples, int32_t out[][2])
{
    const int32_t* t = msaa_table(samples);
    if (!t || !out) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    for (uint32_t s = 0; s < samples; s++) { out[s][0] = t[2 * s]; out[s][1] = t[2 * s + 1]; }
    return SAILOR_HIP_OK;
}

size_t sailor_hip_surface_msaa_bytes(int32_t width, const SailorBand* band, uint32_t samples)
{
    if (!msaa_extent_ok(width, band) || !msaa_table(samples)) return 0;
    return (size_t)band->fbRowCount * (size_t)width * samples * 8;
}

int sailor_hip_surface_msaa_begin(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, void* dStore,
                                  size_t storeBytes, uint32_t samples, const float* dSampleDepthOrNull)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true);
    if (!why) why = msaa_store_why(width, band, dStore, storeBytes, samples);
    if (!why && dSampleDepthOrNull && !aligned(dSampleDepthOrNull, 4)) why = "the sample depth is not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_msaa_begin", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const size_t keys = (size_t)band->fbRowCount * width * samples;
    sailor_launch(ctx, k_surface_msaa_begin, dim3((unsigned)((keys + 255) / 256)), dim3(256), reinterpret_cast<unsigned long long*>(dStore),
                  reinterpret_cast<const uint32_t*>(dSampleDepthOrNull), keys);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_msaa_begin");
    return sailor_hip_surface_begin(ctx, nullptr, width, height, band, dWorkspace, workspaceBytes); // zero keys, empty descriptor slots, the sRGB table
}

int sailor_hip_surface_msaa_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                 const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex,
                                 int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, void* dStore, size_t storeBytes,
                                 uint32_t samples)
{
    static const char* who = "sailor_hip_surface_msaa_draw";
    return surf_draw_launch(ctx, who, SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT, false, k_surface_msaa, "k_surface_msaa", nullptr, nullptr, SurfNoCommand(),
                            [&] { return msaa_draw_refusals(ctx, who, width, band, dStore, storeBytes, samples); }, frame, draw, dInstances, dMaterials, numMaterials, dTextures,
                            numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes, reinterpret_cast<unsigned long long*>(dStore), (int)samples,
                            msaa_pattern(msaa_table(samples) ? samples : 1u));
}

int sailor_hip_surface_msaa_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                      const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                      uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, void* dStore,
                                      size_t storeBytes, uint32_t samples)
{
    static const char* who = "sailor_hip_surface_msaa_draw_gltf";
    return surf_draw_launch(ctx, who, SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, true, k_surface_msaa_gltf, "k_surface_msaa_gltf", nullptr,
                            nullptr, SurfNoCommand(), [&] { return msaa_draw_refusals(ctx, who, width, band, dStore, storeBytes, samples); }, frame, draw, dInstances,
                            dMaterials, numMaterials, dTextures, numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes,
                            reinterpret_cast<unsigned long long*>(dStore), (int)samples, msaa_pattern(msaa_table(samples) ? samples : 1u));
}

int sailor_hip_surface_msaa_layer(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const void* dStore,
                                  size_t storeBytes, uint32_t samples, uint32_t layers, uint32_t k, uint8_t* dWeight, uint8_t* dUncoveredOrNull, uint32_t* dCount,
                                  uint32_t* dClippedOrNull)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true);
    if (!why) why = msaa_store_why(width, band, dStore, storeBytes, samples);
    if (!why) why = msaa_planes_why(samples, layers, k, dWeight, dUncoveredOrNull);
    if (!why && (!aligned(dCount, 4) || (dClippedOrNull && !aligned(dClippedOrNull, 4)))) why = "a counter is NULL or not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_msaa_layer", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_msaa_layer, texel_grid(width, (band->fbRowCount + MSAA_LAYER_ROWS - 1) / MSAA_LAYER_ROWS), dim3(256), dWorkspace,
                  reinterpret_cast<const unsigned long long*>(dStore), (int)samples, layers, k, dWeight, dUncoveredOrNull, dCount, dClippedOrNull, (int)width,
                  (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_msaa_layer");
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_msaa_accumulate(SailorHipContext* ctx, const float* dRadiance, const float* dEmissiveOrNull, const uint8_t* dWeight, const uint8_t* dUncoveredOrNull,
                                       uint32_t samples, uint32_t k, float* dTarget, int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_band_ok(width, height, band) ? nullptr : "the band is not valid for the frame";
    if (!why && !msaa_table(samples)) why = "samples is not 1, 2, 4 or 8";
    if (!why) why = msaa_planes_why(samples, samples, k, dWeight, dUncoveredOrNull);
    if (!why && (!aligned(dRadiance, 16) || !aligned(dTarget, 16) || (dEmissiveOrNull && !aligned(dEmissiveOrNull, 16))))
        why = "radiance or target is NULL, or a colour plane is not 16-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_msaa_accumulate", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_msaa_accumulate, texel_grid(width, band->fbRowCount), dim3(256), reinterpret_cast<const float4*>(dRadiance),
                  reinterpret_cast<const float4*>(dEmissiveOrNull), dWeight, dUncoveredOrNull, (int)samples, k, reinterpret_cast<float4*>(dTarget), (int)width,
                  (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_msaa_accumulate");
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_msaa_store_depth(SailorHipContext* ctx, const void* dStore, size_t storeBytes, uint32_t samples, float* dSampleDepthOutOrNull, float* dDepthOrNull,
                                        int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_band_ok(width, height, band) ? nullptr : "the band is not valid for the frame";
    if (!why) why = msaa_store_why(width, band, dStore, storeBytes, samples);
    if (!why && !dSampleDepthOutOrNull && !dDepthOrNull) why = "both outputs are NULL";
    if (!why && ((dSampleDepthOutOrNull && !aligned(dSampleDepthOutOrNull, 4)) || (dDepthOrNull && !aligned(dDepthOrNull, 4)))) why = "a depth output is not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_msaa_store_depth", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_msaa_store_depth, texel_grid(width, band->fbRowCount), dim3(256), reinterpret_cast<const unsigned long long*>(dStore), (int)samples,
                  dSampleDepthOutOrNull, dDepthOrNull, (int)width, (int)band->fbRowBegin, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_msaa_store_depth");
    return SAILOR_HIP_OK;
}

} // extern "C"
