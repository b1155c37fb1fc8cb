// GPU-driven draws in the surface pass: one command of DrawIndexedIndirect (RHI/GraphicsDriver.h:323) as the reference records every scene draw
// (RHI/Batch.hpp:169, :289).  The host knows the command as it wrote it (Batch.hpp:148-153) -- the un-culled instanceCount is the CAPACITY of the draw --,
// the "GPU Culling" dispatch (ComputeMeshCulling.shader:146-177; sailor_hip_mesh_cull_compact) rewrites instanceCount and compacts the records in place, and
// the draw reads the count where it runs: the host never learns how many instances survive.  include/sailor_hip.h has the pinned rules; tests/indirect_ref.py
// restates them and the kernels are held to the existing restatements of the surviving draws bit for bit.
//
//   k_surface_visibility_indirect        surface_masked_body.h's draw for Standard.shader (with or without ALPHA_CUTOUT), the grid sized from the capacity.
//   k_surface_visibility_indirect_gltf   the same for Standard_glTF.shader.
//
// Each begins with ONE wave-uniform plain load of the command's instanceCount and firstInstance, clamps the count (rule 3) and hands the body a descriptor
// that holds numDrawn = n and firstInstance as read.  From there on the body is what the direct draws run: a lane at or beyond n * numTriangles has no
// triangle (`have` is false: no set-up, no part in the ballots), the descriptor block 0 stores is the clamped one, and order = primBase + 2 * id + part with
// id = d * numTriangles + triangle does not depend on the count.  A block whose first lane is beyond the count leaves right after the load.
#include "surface_masked_body.h"

__global__ __launch_bounds__(256) void k_surface_visibility_indirect(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const uint32_t* __restrict__ command,
                                                                     uint32_t numInstanceRecords, const float* __restrict__ instances,
                                                                     const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                     const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W,
                                                                     int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    if (!surf_indirect_command(draw, command, numInstanceRecords)) return;
    surf_visibility_masked<false>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

__global__ __launch_bounds__(256) void k_surface_visibility_indirect_gltf(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const uint32_t* __restrict__ command,
                                                                          uint32_t numInstanceRecords, const float* __restrict__ instances,
                                                                          const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                                          const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex,
                                                                          int W, int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    if (!surf_indirect_command(draw, command, numInstanceRecords)) return;
    surf_visibility_masked<true>(P, V, draw, instances, materials, numMaterials, textures, numTextures, drawIndex, W, H, rowBegin, rows, workspace);
}

// ---- entry point ----------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int sailor_hip_surface_draw_indirect(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                     const SailorDrawIndexedIndirectData* dCommand, const SailorPerInstanceData* dInstances, uint32_t numInstanceRecords,
                                     const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                     uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    // (the grid and its slices come from the capacity: the count is not known here)
    return surf_draw_launch(ctx, "sailor_hip_surface_draw_indirect", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, false,
                            k_surface_visibility_indirect, "k_surface_visibility_indirect", k_surface_visibility_indirect_gltf, "k_surface_visibility_indirect_gltf",
                            SurfCommand{dCommand, numInstanceRecords}, surf_no_refusals, frame, draw, dInstances, dMaterials, numMaterials, dTextures, numTextures, drawIndex,
                            width, height, band, dWorkspace, workspaceBytes);
}

} // extern "C"
