// The Masked render queue of RenderScene and of the depth prepass: Standard.shader with ALPHA_CUTOUT (:383, :403-408 `if (material.albedo.a < 0.5) discard;`)
// in the visibility-buffer form of surface.hip.  `discard` depends on the fragment's interpolated texcoord, its vertex colour and a texture fetch, so the
// decision is taken in the DRAW, before the key is issued: a discarded fragment writes no key and no depth and takes no part in ties, the resolve and the
// composite stay as they are.  include/sailor_hip.h has the pinned rules; tests/masked_ref.py restates them sequentially and the kernels are held to it bit
// for bit.
//
//   k_surface_visibility_masked  k_surface_visibility's structure (a lane per (instance, triangle); small boxes filled by their lane, large triangles handed
//                                round the wave over 64 x 64 superblocks and 8 x 8 blocks; slices for draws of few triangles) plus the alpha test.  Per fragment:
//                                the exact inside test and z -> the plain relaxed load of the pixel's key -> ONLY a fragment whose key would win evaluates
//                                alpha (two divisions per barycentric, four texel loads) -> only a survivor issues the 64-bit atomicMax.  The owning lane
//                                prepares the alpha words once per triangle (SurfAlpha); for a large triangle they travel with it by __shfl.
//   k_surface_store_depth        a lane per pixel of the band: the key's high word into the band's rows of the whole-frame depth attachment -- the depth
//                                write of a Masked DepthPrepass and of a z-writing RenderScene pass that held cutout draws.
//
// Discard is a pure function of the fragment (its triangle's set-up, the pixel, the material, the texels), so the keys stay order-free: the maximum over the
// surviving fragments does not depend on who issues them or when.
#include "surface_masked_body.h"

// the body (SurfAlpha, the alpha test, the fill) is surface_masked_body.h's, shared with the glTF draw of surface_gltf.hip
__global__ __launch_bounds__(256) void k_surface_visibility_masked(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                                   const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                   const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                                   int rowBegin, int rows, void* __restrict__ workspace)
{
    surf_visibility_masked<false>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_store_depth(const void* __restrict__ workspace, float* __restrict__ depth, int W, int rowBegin, int rows)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    depth[(size_t)(rowBegin + jb) * W + i] = __uint_as_float((unsigned int)(ws.keys[(size_t)jb * W + i] >> 32));
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int sailor_hip_surface_draw_masked(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                   const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                   uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    return surf_draw_launch(ctx, "sailor_hip_surface_draw_masked", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT, false, k_surface_visibility_masked,
                            "k_surface_visibility_masked", nullptr, nullptr, SurfNoCommand(), surf_no_refusals, frame, draw, dInstances, dMaterials, numMaterials, dTextures,
                            numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes);
}

int sailor_hip_surface_store_depth(SailorHipContext* ctx, const void* dWorkspace, size_t workspaceBytes, float* dDepth, int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, false);
    if (!why && !aligned(dDepth, 4)) why = "the depth attachment is NULL or not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_store_depth", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_store_depth, texel_grid(width, band->fbRowCount), dim3(256), dWorkspace, dDepth, (int)width, (int)band->fbRowBegin, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_store_depth");
    return SAILOR_HIP_OK;
}

} // extern "C"
