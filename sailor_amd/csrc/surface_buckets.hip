// The Transparent render queue in ONE rasterisation: per-pixel fragment buckets.  A second mechanism under the rules pinned in include/sailor_hip.h (the
// Transparent section), beside the peel of surface_transparent.hip, whose every layer rasterises the pass again.  Here the draws run once and leave, at every
// pixel, the pixel's first K fragments in primitive order; every layer is then read out of that store into the workspace, and from there on the pass is the
// peel's: the existing resolve, the existing shade, k_surface_blend.  A layer read out of the buckets is the very key the peel's commit would have left, so the
// two routes give the same bits; tests/test_transparent_buckets_gpu.py holds them to it.
//
//   k_surface_bucket, k_surface_bucket_gltf  surface_masked_body.h's draw with SURF_DRAW_BUCKET: a fragment that exists (the Masked queue's), passes
//                                            zbits >= depth[pixel] against the READ-ONLY depth attachment and survives its discard is inserted into the
//                                            pixel's K + 1 slots by surf_fragment_bucket, whose comment holds the store, the insertion and why every
//                                            schedule leaves the same planes.  The workspace only takes the draw's descriptor.
//   k_surface_bucket_layer                   a lane per pixel of 16 rows, as k_surface_peel_commit: plane k's orderPlus1 << 32 | zbits becomes the workspace
//                                            key zbits << 32 | orderPlus1 (an empty slot: 0) and the non-empty pixels are added to a counter, one atomicAdd
//                                            per wave.  For k == K, the sentinel plane, it only counts: the OVERFLOW, the pixels with more than K fragments.
//
// A pass: sailor_hip_surface_bucket_begin (the workspace as sailor_hip_surface_begin leaves it, every slot EMPTY), every draw once, then K times { layer(k),
// resolve, shade, blend }, then layer(K).  The store is (K + 1) x 8 bytes a pixel.
#include "surface_transparent.h"

__global__ __launch_bounds__(256) void k_surface_bucket(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                        const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                        const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                        int rowBegin, int rows, void* __restrict__ workspace, const uint32_t* __restrict__ depth,
                                                        unsigned long long* __restrict__ buckets, uint32_t layers)
{
    SurfBucket b;
    b.depth = depth; b.buckets = buckets; b.plane = (size_t)rows * W; b.layers = layers;
    surf_visibility_masked<false, false, SURF_DRAW_BUCKET>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace, b);
}

__global__ __launch_bounds__(256) void k_surface_bucket_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                             const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                             const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                             int rowBegin, int rows, void* __restrict__ workspace, const uint32_t* __restrict__ depth,
                                                             unsigned long long* __restrict__ buckets, uint32_t layers)
{
    SurfBucket b;
    b.depth = depth; b.buckets = buckets; b.plane = (size_t)rows * W; b.layers = layers;
    surf_visibility_masked<true, false, SURF_DRAW_BUCKET>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace, b);
}

// k_surface_peel_commit's shape and for its reason: a wave adds what it found in 64 texels of 16 rows ONCE.  (No lane leaves before the ballots.)
#define BUCKET_LAYER_ROWS 16
__global__ __launch_bounds__(256) void k_surface_bucket_layer(void* __restrict__ workspace, const unsigned long long* __restrict__ buckets, uint32_t k, uint32_t layers,
                                                              uint32_t* __restrict__ count, int W, int rows)
{
    const int i = texel_i(), j0 = texel_j() * BUCKET_LAYER_ROWS;
    const size_t plane = (size_t)rows * W;
    const SurfWorkspace ws = surf_workspace(workspace, plane);
    const unsigned long long* __restrict__ slots = buckets + (size_t)k * plane;
    uint32_t found = 0;
    for (int r = 0; r < BUCKET_LAYER_ROWS; r++) {
        const int jb = j0 + r;
        const size_t at = (size_t)jb * W + i;
        const bool inside = i < W && jb < rows;
        const unsigned long long key = inside ? slots[at] : SURF_BUCKET_EMPTY;
        const bool has = key != SURF_BUCKET_EMPTY;
        if (inside && k < layers) ws.keys[at] = has ? (key << 32) | (key >> 32) : 0ull;
        found += (uint32_t)__popcll(__ballot(has));
    }
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(count, found);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
#define BUCKET_MAX_LAYERS 64u

// what every entry checks of the store: why not, or NULL.  (The band has been checked by then.)
static const char* bucket_store_why(int32_t width, const SailorBand* band, const void* dBuckets, size_t bucketBytes, uint32_t layers)
{
    if (layers < 1u || layers > BUCKET_MAX_LAYERS) return "layers is outside 1 .. 64";
    if (!aligned(dBuckets, 8)) return "the bucket store is NULL or not 8-byte aligned";
    if (bucketBytes < sailor_hip_surface_bucket_bytes(width, band, layers)) return "the bucket store is smaller than sailor_hip_surface_bucket_bytes";
    return nullptr;
}

// what the two draws refuse beyond surf_draw_prologue (surf_draw_launch's `extra`): the depth attachment, the store, MULTIPLY
static int bucket_draw_refusals(SailorHipContext* ctx, const char* who, const SailorSurfaceDraw* draw, int32_t width, const SailorBand* band, const float* dDepth,
                                const void* dBuckets, size_t bucketBytes, uint32_t layers)
{
    if (!aligned(dDepth, 4)) return surf_refuse(ctx, who, "the depth attachment is NULL or not 4-byte aligned");
    if (const char* why = bucket_store_why(width, band, dBuckets, bucketBytes, layers)) return surf_refuse(ctx, who, why);
    if (peel_is_multiply(draw)) return peel_refuse_multiply(ctx, who);
    return SAILOR_HIP_OK;
}

extern "C" {

size_t sailor_hip_surface_bucket_bytes(int32_t width, const SailorBand* band, uint32_t layers)
{
    if (!band || width <= 0 || width > TEXEL_MAX_EXTENT || band->fbRowCount <= 0 || band->fbRowCount > TEXEL_MAX_EXTENT || layers < 1u || layers > BUCKET_MAX_LAYERS) return 0;
    return ((size_t)layers + 1) * (size_t)band->fbRowCount * (size_t)width * 8;
}

int sailor_hip_surface_bucket_begin(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, void* dBuckets,
                                    size_t bucketBytes, uint32_t layers)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true);
    if (!why) why = bucket_store_why(width, band, dBuckets, bucketBytes, layers);
    if (why) return surf_refuse(ctx, "sailor_hip_surface_bucket_begin", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    SAILOR_TRY_HIP(ctx, hipMemsetAsync(dBuckets, 0xFF, sailor_hip_surface_bucket_bytes(width, band, layers), ctx->stream)); // every slot EMPTY
    return sailor_hip_surface_begin(ctx, nullptr, width, height, band, dWorkspace, workspaceBytes); // zero keys, empty descriptor slots, the sRGB table
}

int sailor_hip_surface_bucket_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                   const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex,
                                   int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth, void* dBuckets,
                                   size_t bucketBytes, uint32_t layers)
{
    static const char* who = "sailor_hip_surface_bucket_draw";
    return surf_draw_launch(ctx, who, SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | PEEL_BLEND_BITS, false, k_surface_bucket, "k_surface_bucket", nullptr, nullptr,
                            SurfNoCommand(), [&] { return bucket_draw_refusals(ctx, who, draw, width, band, dDepth, dBuckets, bucketBytes, layers); }, frame, draw, dInstances,
                            dMaterials, numMaterials, dTextures, numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes,
                            reinterpret_cast<const uint32_t*>(dDepth), reinterpret_cast<unsigned long long*>(dBuckets), layers);
}

int sailor_hip_surface_bucket_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                        const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                        uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth,
                                        void* dBuckets, size_t bucketBytes, uint32_t layers)
{
    static const char* who = "sailor_hip_surface_bucket_draw_gltf";
    return surf_draw_launch(ctx, who, SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF | PEEL_BLEND_BITS, true, k_surface_bucket_gltf,
                            "k_surface_bucket_gltf", nullptr, nullptr, SurfNoCommand(),
                            [&] { return bucket_draw_refusals(ctx, who, draw, width, band, dDepth, dBuckets, bucketBytes, layers); }, frame, draw, dInstances, dMaterials,
                            numMaterials, dTextures, numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes, reinterpret_cast<const uint32_t*>(dDepth),
                            reinterpret_cast<unsigned long long*>(dBuckets), layers);
}

int sailor_hip_surface_bucket_layer(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes,
                                    const void* dBuckets, size_t bucketBytes, uint32_t layers, uint32_t k, uint32_t* dCount)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true);
    if (!why) why = bucket_store_why(width, band, dBuckets, bucketBytes, layers);
    if (!why && k > layers) why = "k is beyond layers";
    if (!why && !aligned(dCount, 4)) why = "the counter is NULL or not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_bucket_layer", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_bucket_layer, texel_grid(width, (band->fbRowCount + BUCKET_LAYER_ROWS - 1) / BUCKET_LAYER_ROWS), dim3(256), dWorkspace,
                  reinterpret_cast<const unsigned long long*>(dBuckets), k, layers, dCount, (int)width, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_bucket_layer");
    return SAILOR_HIP_OK;
}

} // extern "C"
