// RenderScene's producer of the surface buffer: Standard.shader's vertex stage (:126-139), the rasteriser between the stages and the material half of
// the fragment stage (:379-389, :438) as a VISIBILITY BUFFER for gfx950.  include/sailor_hip.h has the pinned rules; tests/surface_ref.py restates them
// sequentially (draw by draw, a >= test against a depth array) and the kernels are held to it bit for bit.
//
//   k_surface_begin       one 64-bit key per pixel of the band = prepass depth bits << 32 (or 0); empty descriptor slots; the sRGB table
//   k_surface_visibility  per draw: a lane per (instance, triangle) sets its triangle up as k_raster_depth does; small triangles are filled by their
//                         lane, large ones are handed round the wave -- the 8 x 8 blocks of a 64 x 64 superblock one per lane, the blocks an edge does
//                         not rule out one lane per texel.  A fragment READS the pixel's key and issues the 64-bit atomicMax only if its own is larger:
//                         behind a prepass almost every losing fragment ends at that plain load.
//   k_surface_resolve     a lane per pixel: key -> draw (binary search of primBase over the descriptors) -> instance, triangle, part; the set-up again,
//                         the edge functions at this pixel, the varyings one by one (never all 54 vertex values at once), material, four samples.  The
//                         body is surface_resolve_body.h's surf_resolve_pixel, shared with k_surface_resolve_gltf and k_surface_resolve_lod.
//   k_surface_composite   target = covered ? radiance : target
//
// The depth of a fragment and everything in front of it (clip, cut, snap, edges, top-left) are raster.hip's, so that the depth is the prepass's bit for
// bit.  The helpers are written once, in raster_prims.h, for both (SurfTri, surf_cut, surf_floor_div256, surf_edge, surf_top_left, surf_bcast64).  raster.hip
// reads tightly packed positions and keeps its own raster_setup; surface_setup (surface_common.h) is that set-up over interleaved vertices, which also
// reports where each vertex came from.  The fill of a set-up triangle is surface_fill.h's, shared with surface_masked.hip (the Masked queue:
// ALPHA_CUTOUT in the draw), surface_gltf.hip (Standard_glTF.shader), surface_indirect.hip and particles.hip.
#include "surface_resolve_body.h"

__global__ __launch_bounds__(256) void k_surface_begin(const float* __restrict__ depth, int W, int rowBegin, int rows, uint32_t maxDraws, void* __restrict__ workspace,
                                                       SurfSrgb table)
{
    const size_t pixels = (size_t)rows * W;
    const SurfWorkspace ws = surf_workspace(workspace, pixels);
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < pixels) ws.keys[g] = depth ? (unsigned long long)__float_as_uint(depth[(size_t)rowBegin * W + g]) << 32 : 0ull;
    if (g < maxDraws) {
        SailorSurfaceDraw e;
        e.dVertices = nullptr; e.dIndices = nullptr; e.dInstanceIds = nullptr;
        e.numTriangles = 0; e.numDrawn = 0; e.primBase = 0xFFFFFFFFu; e.flags = 0; e.firstInstance = 0; e._pad = 0;
        ws.draws[g] = e;
    }
    if (g < 256) ws.srgb[g] = table.v[g];
    if (g == 0) {
        SurfHeader h;
        memset(&h, 0, sizeof h);
        h.maxDraws = maxDraws; h.rows = (uint32_t)rows; h.width = (uint32_t)W; h.fbRowBegin = (uint32_t)rowBegin;
        *ws.header = h;
    }
}

// ---- the draw -------------------------------------------------------------------------------------------------------------------------------------
// gridDim.y SLICES: a draw of few triangles has few waves, and a wave fills its large triangles alone, superblock after superblock (the two triangles of a ground
// quad would be two waves' work, whatever the frame's size).  Such a draw is launched gridDim.y times over: every slice sets all triangles up again (cheap: there are
// few), slice 0 fills the small ones, and of a large triangle's superblocks slice y takes those whose running number is y modulo the slices.  The keys do not
// depend on who writes them.
__global__ __launch_bounds__(256) void k_surface_visibility(Mat4 P, Mat4 V, SailorSurfaceDraw draw, const float* __restrict__ instances, uint32_t drawIndex, int W, int H,
                                                            int rowBegin, int rows, void* __restrict__ workspace)
{
    const SurfWorkspace ws = surf_workspace(workspace, (size_t)rows * W);
    const unsigned int slice = blockIdx.y, slices = gridDim.y;
    if (blockIdx.x == 0 && slice == 0 && threadIdx.x == 0) ws.draws[drawIndex] = draw; // the resolve finds the draw here
    unsigned long long* keys = ws.keys;
    const float* __restrict__ vertices = reinterpret_cast<const float*>(draw.dVertices);
    const unsigned long long total = (unsigned long long)draw.numDrawn * draw.numTriangles;
    const unsigned long long id = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool have = id < total;
    uint32_t d = 0, tri = 0, inst = 0;
    if (have) {
        d = (uint32_t)(id / draw.numTriangles); tri = (uint32_t)(id - (unsigned long long)d * draw.numTriangles);
        inst = draw.dInstanceIds ? draw.dInstanceIds[d] : draw.firstInstance + d;
    }
    const bool cullBack = (draw.flags & SAILOR_SURFACE_CULL_BACK) != 0;
    // a triangle cut by the near plane can leave a quad: its second half is a second trip through the same code, taken only by waves that hold one
    bool again = false;
    for (int part = 0; part < 2; part++) {
        if (part && !__any(again)) break;
        SurfTri t;
        t.valid = false;
        bool second = false;
        if (have && (part == 0 || again)) {
            SurfSrc S;
            t = surface_setup(P, V, instances + SURF_INSTANCE_FLOATS * (size_t)inst, vertices, draw.dIndices + 3 * (size_t)tri, W, H, rowBegin, rowBegin + rows, cullBack,
                              part, second, S);
        }
        const unsigned int orderPlus1 = draw.primBase + (unsigned int)(2ull * id) + (unsigned int)part + 1u; // (the entry point has checked the range)
        surf_fill(t, orderPlus1, SurfNoPayload(), SurfNoBcast(), slice, slices, lane, [&](int i, int j, float z, unsigned int tag, auto&&...) {
            surf_fragment(keys + (size_t)(j - rowBegin) * W + i, z, tag);
        });
        if (part == 0) again = second;
    }
}

// ---- the resolve (surf_resolve_pixel: surface_resolve_body.h; Standard.shader alone, no occlusion or emissive plane) ---------------------------------

__global__ __launch_bounds__(256) void k_surface_resolve(Mat4 P, Mat4 V, const float* __restrict__ instances, const SailorMaterialData* __restrict__ materials,
                                                         uint32_t numMaterials, const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, int W, int H,
                                                         int rowBegin, int rows, uint32_t maxDraws, const void* __restrict__ workspace, float4* __restrict__ surface, size_t planeStride,
                                                         float* __restrict__ depthOut, uint8_t* __restrict__ coverage)
{
    surf_resolve_pixel<false, false>(P, V, instances, materials, numMaterials, textures, numTextures, W, H, rowBegin, rows, maxDraws, workspace, surface, planeStride, depthOut,
                                     coverage, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_surface_composite(const float4* __restrict__ radiance, const void* __restrict__ workspace, float4* __restrict__ target, int W, int rows)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    const size_t at = (size_t)jb * W + i;
    if ((unsigned int)ws.keys[at] != 0u) target[at] = radiance[at];
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------

extern "C" {

int sailor_host_srgb_table(float out[256])
{
    if (!out) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 256; i++) {
        const double c = (double)i / 255.0;
        out[i] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
    return SAILOR_HIP_OK;
}

size_t sailor_hip_surface_keys_offset(void) { return (size_t)SURF_HEADER_BYTES + SURF_TABLE_BYTES; }

int sailor_hip_surface_draw_prims(uint32_t numTriangles, uint32_t numDrawn, uint64_t* out)
{
    if (!out) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const uint64_t n = (uint64_t)numDrawn * (uint64_t)numTriangles;
    *out = n > 0x7FFFFFFFFFFFFFFFull ? 0xFFFFFFFFFFFFFFFFull : 2ull * n; // saturates
    return SAILOR_HIP_OK;
}

size_t sailor_hip_surface_workspace_bytes(int32_t width, int32_t height, const SailorBand* band, uint32_t maxDraws)
{
    if (!surf_band_ok(width, height, band) || maxDraws == 0 || maxDraws > SURF_MAX_DRAWS) return 0;
    return surf_fixed_bytes(width, band) + (size_t)maxDraws * sizeof(SailorSurfaceDraw);
}

int sailor_hip_surface_begin(SailorHipContext* ctx, const float* dDepthOrNull, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace,
                             size_t workspaceBytes)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    uint32_t maxDraws = 0;
    if (const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true, &maxDraws)) return surf_refuse(ctx, "sailor_hip_surface_begin", why);
    static const SurfSrgb table = [] { SurfSrgb t; sailor_host_srgb_table(t.v); return t; }();
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pixels = (size_t)band->fbRowCount * width;
    size_t threads = pixels > maxDraws ? pixels : maxDraws;
    if (threads < 256) threads = 256;
    sailor_launch(ctx, k_surface_begin, dim3((unsigned)((threads + 255) / 256)), dim3(256), dDepthOrNull, (int)width, (int)band->fbRowBegin, (int)band->fbRowCount, maxDraws,
                  dWorkspace, table);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_begin");
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                            uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    SurfDrawSetup s;
    if (const int st = surf_draw_prologue(ctx, "sailor_hip_surface_draw", SAILOR_SURFACE_CULL_BACK, false, nullptr, frame, draw, dInstances, false, drawIndex, width, height,
                                          band, dWorkspace, workspaceBytes, s))
        return st;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_visibility, s.grid, dim3(256), s.P, s.V, *draw, reinterpret_cast<const float*>(dInstances), drawIndex, (int)width, (int)height,
                  (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_visibility");
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_resolve(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials,
                               uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, int32_t width, int32_t height, const SailorBand* band,
                               const void* dWorkspace, size_t workspaceBytes, float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull)
{
    return surf_resolve_launch(ctx, "sailor_hip_surface_resolve", k_surface_resolve, "k_surface_resolve", frame, dInstances, dMaterials, numMaterials, dTextures, numTextures,
                               width, height, band, dWorkspace, workspaceBytes, dSurface, planeStride, dDepthOutOrNull, dCoverageOrNull);
}

int sailor_hip_surface_composite(SailorHipContext* ctx, const float* dRadiance, const void* dWorkspace, size_t workspaceBytes, float* dTarget, int32_t width,
                                 int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, false);
    if (!why && (!aligned(dRadiance, 16) || !aligned(dTarget, 16))) why = "radiance or target is NULL or not 16-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_composite", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_composite, texel_grid(width, band->fbRowCount), dim3(256), reinterpret_cast<const float4*>(dRadiance), dWorkspace,
                  reinterpret_cast<float4*>(dTarget), (int)width, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_composite");
    return SAILOR_HIP_OK;
}

} // extern "C"
