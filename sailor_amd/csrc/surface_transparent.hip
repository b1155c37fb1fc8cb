// The Transparent render queue of RenderScene: draws with depth test on and z-write OFF whose fragments are blended in Vulkan's primitive order
// (ModelImporter.cpp:213-229 for alphaMode BLEND, MaterialImporter.cpp:329-357 for a .mat file's blendMode, VulkanPipileneStates.cpp:236-254 for the
// states).  A visibility buffer keeps one fragment per pixel, a blended pass needs every fragment that passes the depth test: the pass is PEELED BY
// PRIMITIVE ORDER, one layer at a time.  Layer k holds, at each pixel, that pixel's k-th fragment in primitive order; it goes through the existing
// resolve and the existing shade and then through the blend.  include/sailor_hip.h has the pinned rules; tests/transparent_ref.py restates them
// sequentially and the kernels are held to it bit for bit.
//
//   k_surface_peel, k_surface_peel_gltf  surface_masked_body.h's draw with PEEL: a fragment that exists (set-up, cut, snap, cull, top-left, fill: the Masked
//                                        queue's), passes zbits >= depth[pixel] against the READ-ONLY depth attachment and lies beyond last[pixel] issues
//                                        (0xFFFFFFFF - orderPlus1) << 32 | zbits by plain load, discard, atomicMax: the maximum is the smallest order beyond
//                                        the previous layer, whoever issues it and whenever.
//   k_surface_peel_commit                a lane per pixel of 16 rows: a non-zero key becomes the standard zbits << 32 | orderPlus1, last[pixel] = orderPlus1,
//                                        and the pixels committed are added to a counter, one atomicAdd per wave behind its ballots.  After it the workspace
//                                        is an ordinary surface workspace: the resolves and the shade run on it unchanged.
//   k_surface_blend                      a lane per pixel: the owning draw by the resolve's binary search (surf_owning_draw, surface_resolve_body.h), its blend
//                                        mode, one load and one store of the target.
//
// A pass of L layers re-rasterises its draws L + 1 times (the last time only counts what is left): the price of reusing the resolve and the shade.
// (surface_buckets.hip is the route that rasterises once; it ends in the same resolve, shade and k_surface_blend.)
#include "surface_transparent.h"
#include "surface_resolve_body.h"

__global__ __launch_bounds__(256) void k_surface_peel(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                      const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                      const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H, int rowBegin,
                                                      int rows, void* __restrict__ workspace, const uint32_t* __restrict__ depth, const uint32_t* __restrict__ last)
{
    SurfPeel peel;
    peel.depth = depth; peel.last = last;
    surf_visibility_masked<false, false, SURF_DRAW_PEEL>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace, peel);
}

__global__ __launch_bounds__(256) void k_surface_peel_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                           const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                           const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                           int rowBegin, int rows, void* __restrict__ workspace, const uint32_t* __restrict__ depth,
                                                           const uint32_t* __restrict__ last)
{
    SurfPeel peel;
    peel.depth = depth; peel.last = last;
    surf_visibility_masked<true, false, SURF_DRAW_PEEL>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace, peel);
}

// A wave takes 64 texels of PEEL_COMMIT_ROWS rows one after the other and adds what it committed ONCE: every atomicAdd lands on one word, and a wave per
// 64 texels (130 000 atomics at 3840 x 2160) made the kernel 1.47 ms of waiting for them.  (No lane leaves before the ballots: lane 0 of the wave issues the add.)
#define PEEL_COMMIT_ROWS 16
__global__ __launch_bounds__(256) void k_surface_peel_commit(void* __restrict__ workspace, uint32_t* __restrict__ last, uint32_t* __restrict__ count, int W, int rows)
{
    const int i = texel_i(), j0 = texel_j() * PEEL_COMMIT_ROWS;
    const SurfWorkspace ws = surf_workspace(workspace, (size_t)rows * W);
    uint32_t committed = 0;
    for (int r = 0; r < PEEL_COMMIT_ROWS; r++) {
        const int jb = j0 + r;
        const size_t at = (size_t)jb * W + i;
        unsigned long long key = 0ull;
        if (i < W && jb < rows) key = ws.keys[at];
        const bool has = key != 0ull;
        if (has) {
            const unsigned int orderPlus1 = 0xFFFFFFFFu - (unsigned int)(key >> 32);
            ws.keys[at] = ((key & 0xFFFFFFFFull) << 32) | orderPlus1;
            last[at] = orderPlus1;
        }
        committed += (uint32_t)__popcll(__ballot(has));
    }
    if ((threadIdx.x & 63) == 0 && committed) atomicAdd(count, committed);
}

// rule 4 of the Transparent section, one fp32 rounding per written operation (the library is built without contraction): the source products first, then the
// destination's, then the add or the subtract (VulkanPipileneStates.cpp:236-247; the alpha op of AlphaBlending is SUBTRACT, as in k_sky_blit_clouds)
__device__ __forceinline__ float4 surf_blend(uint32_t mode, const float4 src, const float4 dst)
{
    if (mode == SAILOR_SURFACE_BLEND_ADDITIVE) return make_float4(src.x + dst.x, src.y + dst.y, src.z + dst.z, src.w + dst.w);
    if (mode == SAILOR_SURFACE_BLEND_ALPHA) {
        const float k = 1.0f - src.w;
        return make_float4(src.x * src.w + dst.x * k, src.y * src.w + dst.y * k, src.z * src.w + dst.z * k, src.w * src.w - dst.w * k);
    }
    return src;
}

__global__ __launch_bounds__(256) void k_surface_blend(const float4* __restrict__ radiance, const float4* __restrict__ surfaceP0, const float4* __restrict__ emissive,
                                                       const void* __restrict__ workspace, uint32_t maxDraws, float4* __restrict__ target, int W, int rows)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    const size_t at = (size_t)jb * W + i;
    const unsigned int low = (unsigned int)ws.keys[at];
    if (low == 0u) return;
    SailorSurfaceDraw draw; // (the pixel went through the resolve: of what the search reports only the draw's flags are read here)
    unsigned int instance, rest;
    surf_owning_draw(ws, maxDraws, low - 1u, draw, instance, rest);
    const uint32_t mode = (draw.flags >> SAILOR_SURFACE_BLEND_SHIFT) & SAILOR_SURFACE_BLEND_MASK;
    const float4 r = radiance[at];
    float4 src = make_float4(r.x, r.y, r.z, surfaceP0[at].w);
    if (emissive) {
        const float4 e = emissive[at];
        src.x = e.x + r.x; src.y = e.y + r.y; src.z = e.z + r.z; // k_surface_composite_gltf's sum
    }
    target[at] = surf_blend(mode, src, target[at]);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
// what the two peel draws refuse beyond surf_draw_prologue (surf_draw_launch's `extra`): the two planes, then MULTIPLY
static int peel_draw_refusals(SailorHipContext* ctx, const char* who, const SailorSurfaceDraw* draw, const float* dDepth, const uint32_t* dLast)
{
    if (!aligned(dDepth, 4)) return surf_refuse(ctx, who, "the depth attachment is NULL or not 4-byte aligned");
    if (!aligned(dLast, 4)) return surf_refuse(ctx, who, "the last-order plane is NULL or not 4-byte aligned");
    if (peel_is_multiply(draw)) return peel_refuse_multiply(ctx, who);
    return SAILOR_HIP_OK;
}

extern "C" {

int sailor_hip_surface_peel_begin(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, uint32_t* dLast,
                                  int32_t startPass)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true);
    if (!why && !aligned(dLast, 4)) why = "the last-order plane is NULL or not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_peel_begin", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (startPass) SAILOR_TRY_HIP(ctx, hipMemsetAsync(dLast, 0, (size_t)band->fbRowCount * width * 4, ctx->stream));
    return sailor_hip_surface_begin(ctx, nullptr, width, height, band, dWorkspace, workspaceBytes); // zero keys, empty descriptor slots, the sRGB table
}

int sailor_hip_surface_peel_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                 const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, uint32_t drawIndex,
                                 int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth, const uint32_t* dLast)
{
    static const char* who = "sailor_hip_surface_peel_draw";
    return surf_draw_launch(ctx, who, SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | PEEL_BLEND_BITS, false, k_surface_peel, "k_surface_peel", nullptr, nullptr,
                            SurfNoCommand(), [&] { return peel_draw_refusals(ctx, who, draw, dDepth, dLast); }, frame, draw, dInstances, dMaterials, numMaterials, dTextures,
                            numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes, reinterpret_cast<const uint32_t*>(dDepth), dLast);
}

int sailor_hip_surface_peel_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                      const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                      uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, const float* dDepth,
                                      const uint32_t* dLast)
{
    static const char* who = "sailor_hip_surface_peel_draw_gltf";
    return surf_draw_launch(ctx, who, SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF | PEEL_BLEND_BITS, true, k_surface_peel_gltf,
                            "k_surface_peel_gltf", nullptr, nullptr, SurfNoCommand(), [&] { return peel_draw_refusals(ctx, who, draw, dDepth, dLast); }, frame, draw, dInstances,
                            dMaterials, numMaterials, dTextures, numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes,
                            reinterpret_cast<const uint32_t*>(dDepth), dLast);
}

int sailor_hip_surface_peel_commit(SailorHipContext* ctx, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, uint32_t* dLast,
                                   uint32_t* dCount)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true);
    if (!why && !aligned(dLast, 4)) why = "the last-order plane is NULL or not 4-byte aligned";
    if (!why && !aligned(dCount, 4)) why = "the counter is NULL or not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_peel_commit", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_peel_commit, texel_grid(width, (band->fbRowCount + PEEL_COMMIT_ROWS - 1) / PEEL_COMMIT_ROWS), dim3(256), dWorkspace, dLast, dCount,
                  (int)width, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_peel_commit");
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_blend(SailorHipContext* ctx, const float* dRadiance, const float* dSurfaceP0, const float* dEmissiveOrNull, const void* dWorkspace,
                             size_t workspaceBytes, float* dTarget, int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    uint32_t maxDraws = 0;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, false, &maxDraws);
    if (!why && (!aligned(dRadiance, 16) || !aligned(dSurfaceP0, 16) || !aligned(dTarget, 16))) why = "radiance, the surface's first plane or target is NULL or not 16-byte aligned";
    if (!why && dEmissiveOrNull && !aligned(dEmissiveOrNull, 16)) why = "the emissive plane is not 16-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_blend", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_blend, texel_grid(width, band->fbRowCount), dim3(256), reinterpret_cast<const float4*>(dRadiance), reinterpret_cast<const float4*>(dSurfaceP0),
                  reinterpret_cast<const float4*>(dEmissiveOrNull), dWorkspace, maxDraws, reinterpret_cast<float4*>(dTarget), (int)width, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_blend");
    return SAILOR_HIP_OK;
}

} // extern "C"
