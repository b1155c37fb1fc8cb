// Mip-mapped material textures in the surface pass: every texture() of Standard.shader and Standard_glTF.shader at its implicit level of detail
// (VulkanSamplers.cpp:37-40: mipmapMode LINEAR, no bias), the fetch behind ALPHA_CUTOUT included.  include/sailor_hip.h (the mip-mapped section) has the
// pinned rules, surface_lod.h the level selection; tests/lod_ref.py restates them sequentially and the kernels are held to it bit for bit.
//
//   k_surface_visibility_lod[_gltf]            surface_masked_body.h's draw with LOD = true: a fragment that would win its pixel evaluates uv at its quad's
//                                              other centres from affine steps of its own edge functions and tests the trilinear alpha.
//   k_surface_visibility_indirect_lod[_gltf]   the same behind the command load of surface_indirect.hip.
//   k_surface_resolve_lod                      surface_resolve_body.h's surf_resolve_pixel with LOD: k_surface_resolve_gltf's lines plus uv at the row mate and
//                                              the column mate of the pixel, the four derivatives, and every fetch through surf_texture_lod.  A table of
//                                              one-level descriptors gives k_surface_resolve_gltf's bits.
#include "surface_resolve_body.h"

__global__ __launch_bounds__(256) void k_surface_visibility_lod(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                                const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                                int rowBegin, int rows, void* __restrict__ workspace)
{
    surf_visibility_masked<false, true>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_visibility_lod_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                                     const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                     const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W,
                                                                     int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    surf_visibility_masked<true, true>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_visibility_indirect_lod(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const uint32_t* __restrict__ command,
                                                                         uint32_t numInstanceRecords, const float* __restrict__ instances,
                                                                         const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                         const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex,
                                                                         int W, int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    if (!surf_indirect_command(draw, command, numInstanceRecords)) return;
    surf_visibility_masked<false, true>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_visibility_indirect_lod_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const uint32_t* __restrict__ command,
                                                                              uint32_t numInstanceRecords, const float* __restrict__ instances,
                                                                              const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                              const SailorTextureDesc* __restrict__ textures, uint32_t numTextures,
                                                                              uint32_t drawIndex, int W, int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    if (!surf_indirect_command(draw, command, numInstanceRecords)) return;
    surf_visibility_masked<true, true>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_resolve_lod(Mat4 P, Mat4 V, const float* __restrict__ instances, const SailorMaterialData* __restrict__ materials,
                                                             uint32_t numMaterials, const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, int W, int H,
                                                             int rowBegin, int rows, uint32_t maxDraws, const void* __restrict__ workspace, float4* __restrict__ surface,
                                                             size_t planeStride, float* __restrict__ depthOut, uint8_t* __restrict__ coverage, const float* aoIn,
                                                             float* aoOut, float4* __restrict__ emissive)
{
    surf_resolve_pixel<true, true>(P, V, instances, materials, numMaterials, textures, numTextures, W, H, rowBegin, rows, maxDraws, workspace, surface, planeStride, depthOut,
                                   coverage, aoIn, aoOut, emissive);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int sailor_hip_surface_draw_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    return surf_draw_launch(ctx, "sailor_hip_surface_draw_lod", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, false, k_surface_visibility_lod,
                            "k_surface_visibility_lod", k_surface_visibility_lod_gltf, "k_surface_visibility_lod_gltf", SurfNoCommand(), surf_no_refusals, frame, draw, dInstances,
                            dMaterials, numMaterials, dTextures, numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes);
}

int sailor_hip_surface_draw_indirect_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                         const SailorDrawIndexedIndirectData* dCommand, const SailorPerInstanceData* dInstances, uint32_t numInstanceRecords,
                                         const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                         uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    return surf_draw_launch(ctx, "sailor_hip_surface_draw_indirect_lod", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, false,
                            k_surface_visibility_indirect_lod, "k_surface_visibility_indirect_lod", k_surface_visibility_indirect_lod_gltf,
                            "k_surface_visibility_indirect_lod_gltf", SurfCommand{dCommand, numInstanceRecords}, surf_no_refusals, frame, draw, dInstances, dMaterials, numMaterials,
                            dTextures, numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes);
}

int sailor_hip_surface_resolve_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials,
                                   uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, int32_t width, int32_t height, const SailorBand* band,
                                   const void* dWorkspace, size_t workspaceBytes, float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull,
                                   const float* dAoInOrNull, float* dAoOutOrNull, float* dEmissive)
{
    return surf_resolve_launch(ctx, "sailor_hip_surface_resolve_lod", k_surface_resolve_lod, "k_surface_resolve_lod", frame, dInstances, dMaterials, numMaterials, dTextures,
                               numTextures, width, height, band, dWorkspace, workspaceBytes, dSurface, planeStride, dDepthOutOrNull, dCoverageOrNull, dAoInOrNull, dAoOutOrNull,
                               reinterpret_cast<float4*>(dEmissive));
}

} // extern "C"
