// glTF materials in the surface pass: Standard_glTF.shader, the shader ModelImporter.cpp:156-231 gives every imported model, where it differs from
// Standard.shader -- the normal matrix of the tangent basis (:136-138), the material record (:42-58), the orm / occlusion / emissive fetches (:389-396), the
// emissive term (:399) and alphaCutoff (:411).  include/sailor_hip.h has the pinned rules; tests/gltf_ref.py restates them sequentially and the kernels are
// held to it bit for bit.  The shade kernels are not touched: the resolve here produces their inputs and the composite adds the emissive term behind them.
//
//   k_surface_visibility_gltf  surface_masked_body.h's draw, instantiated for the glTF record: baseColorFactor[3] through baseColorSampler against the
//                              material's alphaCutoff.  Without ALPHA_CUTOUT the keys are k_surface_visibility's.
//   k_surface_resolve_gltf     surface_resolve_body.h's surf_resolve_pixel for a pass that mixes both shaders (MIXED): the owning draw's flag picks the record a
//                              material slot is read as, the matrix under the tangent basis (mat3(model) or its inverse transpose) and the fetches.  A pixel
//                              of a Standard draw computes exactly k_surface_resolve's operations: they are the same lines.  Next to the three planes it writes
//                              the emissive plane and the occlusion the shade is to read (min(g_AO, occlusion texel)).
//   k_surface_composite_gltf   target = covered ? (emissive.rgb + radiance.rgb, radiance.a) : target
#include "surface_resolve_body.h"

__global__ __launch_bounds__(256) void k_surface_visibility_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances,
                                                                 const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                 const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                                 int rowBegin, int rows, void* __restrict__ workspace)
{
    surf_visibility_masked<true>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_resolve_gltf(Mat4 P, Mat4 V, const float* __restrict__ instances, const SailorMaterialData* __restrict__ materials,
                                                              uint32_t numMaterials, const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, int W, int H,
                                                              int rowBegin, int rows, uint32_t maxDraws, const void* __restrict__ workspace, float4* __restrict__ surface,
                                                              size_t planeStride, float* __restrict__ depthOut, uint8_t* __restrict__ coverage, const float* aoIn,
                                                              float* aoOut, float4* __restrict__ emissive)
{
    surf_resolve_pixel<true, false>(P, V, instances, materials, numMaterials, textures, numTextures, W, H, rowBegin, rows, maxDraws, workspace, surface, planeStride, depthOut,
                                    coverage, aoIn, aoOut, emissive);
}

__global__ __launch_bounds__(256) void k_surface_composite_gltf(const float4* __restrict__ radiance, const float4* __restrict__ emissive, const void* __restrict__ workspace,
                                                                float4* __restrict__ target, int W, int rows)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    const size_t at = (size_t)jb * W + i;
    if ((unsigned int)ws.keys[at] != 0u) {
        const float4 r = radiance[at], e = emissive[at];
        target[at] = make_float4(e.x + r.x, e.y + r.y, e.z + r.z, r.w);
    }
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int sailor_hip_surface_draw_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                 const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                 uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    return surf_draw_launch(ctx, "sailor_hip_surface_draw_gltf", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, true, k_surface_visibility_gltf,
                            "k_surface_visibility_gltf", nullptr, nullptr, SurfNoCommand(), surf_no_refusals, frame, draw, dInstances, dMaterials, numMaterials, dTextures,
                            numTextures, drawIndex, width, height, band, dWorkspace, workspaceBytes);
}

int sailor_hip_surface_resolve_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials,
                                    uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, int32_t width, int32_t height, const SailorBand* band,
                                    const void* dWorkspace, size_t workspaceBytes, float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull,
                                    const float* dAoInOrNull, float* dAoOutOrNull, float* dEmissive)
{
    return surf_resolve_launch(ctx, "sailor_hip_surface_resolve_gltf", k_surface_resolve_gltf, "k_surface_resolve_gltf", frame, dInstances, dMaterials, numMaterials, dTextures,
                               numTextures, width, height, band, dWorkspace, workspaceBytes, dSurface, planeStride, dDepthOutOrNull, dCoverageOrNull, dAoInOrNull, dAoOutOrNull,
                               reinterpret_cast<float4*>(dEmissive));
}

int sailor_hip_surface_composite_gltf(SailorHipContext* ctx, const float* dRadiance, const float* dEmissive, const void* dWorkspace, size_t workspaceBytes,
                                      float* dTarget, int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, false);
    if (!why && (!aligned(dRadiance, 16) || !aligned(dEmissive, 16) || !aligned(dTarget, 16))) why = "radiance, emissive or target is NULL or not 16-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_composite_gltf", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_composite_gltf, texel_grid(width, band->fbRowCount), dim3(256), reinterpret_cast<const float4*>(dRadiance),
                  reinterpret_cast<const float4*>(dEmissive), dWorkspace, reinterpret_cast<float4*>(dTarget), (int)width, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_composite_gltf");
    return SAILOR_HIP_OK;
}

} // extern "C"
