// Mip-mapped material textures in the surface pass: every texture() of Standard.shader and Standard_glTF.shader at its implicit level of detail
// (VulkanSamplers.cpp:37-40: mipmapMode LINEAR, no bias), the fetch behind ALPHA_CUTOUT included.  include/sailor_hip.h (the mip-mapped section) has the
// pinned rules, surface_lod.h the level selection; tests/lod_ref.py restates them sequentially and the kernels are held to it bit for bit.
//
//   k_surface_visibility_lod[_gltf]            surface_masked_body.h's draw with LOD = true: a fragment that would win its pixel evaluates uv at its quad's
//                                              other centres from affine steps of its own edge functions and tests the trilinear alpha.
//   k_surface_visibility_indirect_lod[_gltf]   the same behind the command load of surface_indirect.hip.
//   k_surface_resolve_lod                      k_surface_resolve_gltf with uv at the row mate and the column mate of the pixel, the four derivatives, and
//                                              every fetch through surf_texture_lod.  A table of one-level descriptors gives k_surface_resolve_gltf's bits.
#include "surface_masked_body.h"

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
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    const size_t at = (size_t)jb * W + i;
    const unsigned long long key = ws.keys[at];
    const unsigned int low = (unsigned int)key;
    if (depthOut) depthOut[at] = __uint_as_float((unsigned int)(key >> 32));
    float4 p0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p1 = make_float4(0.0f, 0.0f, 1.0f, 1.0f), p2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 em = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    float ao = aoIn ? aoIn[at] : 1.0f;
    bool covered = false;
    if (low != 0u) {
        const unsigned int order = low - 1u;
        unsigned int lo = 0, hi = maxDraws;
        while (hi - lo > 1u) {
            const unsigned int mid = lo + ((hi - lo) >> 1);
            if (ws.draws[mid].primBase <= order) lo = mid; else hi = mid;
        }
        const SailorSurfaceDraw draw = ws.draws[lo];
        const unsigned int rel = order - draw.primBase;
        const unsigned int per = 2u * draw.numTriangles;
        const unsigned int d = per ? rel / per : 0xFFFFFFFFu;
        if (draw.primBase <= order && d < draw.numDrawn) {
            const unsigned int r = rel - d * per, tri = r >> 1;
            const int part = (int)(r & 1u);
            const bool gltf = (draw.flags & SAILOR_SURFACE_GLTF) != 0;
            const uint32_t inst = draw.dInstanceIds ? draw.dInstanceIds[d] : draw.firstInstance + d;
            const float* __restrict__ model = instances + SURF_INSTANCE_FLOATS * (size_t)inst;
            const float* __restrict__ vertices = reinterpret_cast<const float*>(draw.dVertices);
            bool second;
            SurfSrc S;
            const SurfTri t = surface_setup(P, V, model, vertices, draw.dIndices + 3 * (size_t)tri, W, H, rowBegin, rowBegin + rows,
                                            (draw.flags & SAILOR_SURFACE_CULL_BACK) != 0, part, second, S);
            if (t.valid) {
                covered = true;
                const int j = jb + rowBegin;
                const long long px = 256ll * i + 128, py = 256ll * j + 128;
                const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
                const long long e0 = surf_edge(t.x1, t.y1, t.x2, t.y2, px, py), e1 = surf_edge(t.x2, t.y2, t.x0, t.y0, px, py),
                                e2 = surf_edge(t.x0, t.y0, t.x1, t.y1, px, py);
                const float l0 = (float)e0 / area, l1 = (float)e1 / area, l2 = (float)e2 / area;
                const float q0 = l0 / S.w[0], q1 = l1 / S.w[1], q2 = l2 / S.w[2];
                const float s = (q0 + q1) + q2;
                const float b0 = q0 / s, b1 = q1 / s, b2 = q2 / s;
                const float* __restrict__ vI0 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[0];
                const float* __restrict__ vI1 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[1];
                const float* __restrict__ vI2 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[2];
                const float* __restrict__ vO1 = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[1];
                const float* __restrict__ vO2 = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[2];
                float n[9];
                surf_basis_matrix(model, gltf, n);
                float a[18];
                float U[3], Vv[3]; // the three set-up vertices' texcoords, the cut lerp applied: what uv at the quad's other centres needs
#pragma unroll
                for (int c = 0; c < 18; c++) {
                    const float a0 = surf_varying_basis(vI0, model, n, c);
                    float a1 = surf_varying_basis(vI1, model, n, c), a2 = surf_varying_basis(vI2, model, n, c);
                    if (S.cut[1]) a1 = a1 + (surf_varying_basis(vO1, model, n, c) - a1) * S.t[1];
                    if (S.cut[2]) a2 = a2 + (surf_varying_basis(vO2, model, n, c) - a2) * S.t[2];
                    if (c == 0) { U[0] = a0; U[1] = a1; U[2] = a2; }
                    if (c == 1) { Vv[0] = a0; Vv[1] = a1; Vv[2] = a2; }
                    a[c] = (a0 * b0 + a1 * b1) + a2 * b2;
                }
                const float u = a[0], v = a[1];
                // rule 3: uv at the row mate (i ^ 1, j) and the column mate (i, j ^ 1), inside the triangle and the frame or not
                SurfDerivs dv;
                {
                    const long long mx = 256ll * (i ^ 1) + 128, my = 256ll * (j ^ 1) + 128;
                    float ux, vx, uy, vy;
                    surf_uv_at(U, Vv, S.w, surf_edge(t.x1, t.y1, t.x2, t.y2, mx, py), surf_edge(t.x2, t.y2, t.x0, t.y0, mx, py), surf_edge(t.x0, t.y0, t.x1, t.y1, mx, py),
                               area, ux, vx);
                    surf_uv_at(U, Vv, S.w, surf_edge(t.x1, t.y1, t.x2, t.y2, px, my), surf_edge(t.x2, t.y2, t.x0, t.y0, px, my), surf_edge(t.x0, t.y0, t.x1, t.y1, px, my),
                               area, uy, vy);
                    dv = surf_derivs(i, j, u, v, ux, vx, uy, vy);
                }
                const uint32_t mi = reinterpret_cast<const uint32_t*>(model)[20];
                const SailorMaterialData* __restrict__ sm = materials + (mi < numMaterials ? mi : 0u);
                const SailorGltfMaterialData* __restrict__ gm = reinterpret_cast<const SailorGltfMaterialData*>(sm);
                {
                    const float4 tA = surf_texture_lod(textures, numTextures, gltf ? gm->baseColorSampler : sm->albedoSampler, ws.srgb, u, v, dv);
                    p2.x = (sm->albedo[0] * tA.x) * a[5]; p2.y = (sm->albedo[1] * tA.y) * a[6]; p2.z = (sm->albedo[2] * tA.z) * a[7];
                    p0 = make_float4(a[2], a[3], a[4], (sm->albedo[3] * tA.w) * a[8]);
                }
                {
                    const float4 tO = surf_texture_lod(textures, numTextures, gltf ? gm->ormSampler : sm->metalnessSampler, ws.srgb, u, v, dv);
                    if (gltf) {
                        p2.w = gm->metallicFactor * tO.z;
                        p1.w = gm->roughnessFactor * tO.y;
                    } else {
                        p2.w = sm->metallic * tO.x;
                        p1.w = sm->roughness * surf_texture_lod(textures, numTextures, sm->roughnessSampler, ws.srgb, u, v, dv).x;
                    }
                }
                if (gltf) {
                    const float tOcc = surf_texture_lod(textures, numTextures, gm->occlusionSampler, ws.srgb, u, v, dv).x;
                    const float4 tE = surf_texture_lod(textures, numTextures, gm->emissiveSampler, ws.srgb, u, v, dv);
                    em = make_float4(gm->emissiveFactor[0] * tE.x, gm->emissiveFactor[1] * tE.y, gm->emissiveFactor[2] * tE.z, tOcc);
                    ao = (tOcc < ao) ? tOcc : ao;
                }
                const float4 tN = surf_texture_lod(textures, numTextures, gltf ? gm->normalSampler : sm->normalSampler, ws.srgb, u, v, dv);
                float nx = 2.0f * tN.x - 1.0f, ny = 2.0f * tN.y - 1.0f, nz = 2.0f * tN.z - 1.0f;
                float len = sqrtf(dot3f(nx, ny, nz, nx, ny, nz));
                nx = nx / len; ny = ny / len; nz = nz / len;
                if (gltf) {
                    const float scale = gm->normalScale;
                    nx = nx * scale; ny = ny * scale; nz = nz * scale;
                }
                float wx = (a[9] * nx + a[12] * ny) + a[15] * nz, wy = (a[10] * nx + a[13] * ny) + a[16] * nz, wz = (a[11] * nx + a[14] * ny) + a[17] * nz;
                len = sqrtf(dot3f(wx, wy, wz, wx, wy, wz));
                p1.x = wx / len; p1.y = wy / len; p1.z = wz / len;
            }
        }
    }
    surface[at] = p0;
    surface[planeStride + at] = p1;
    surface[2 * planeStride + at] = p2;
    emissive[at] = em;
    if (aoOut) aoOut[at] = ao;
    if (coverage) coverage[at] = covered ? 1 : 0;
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int sailor_hip_surface_draw_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances,
                                const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    SurfDrawSetup s;
    if (const int st = surf_draw_prologue(ctx, "sailor_hip_surface_draw_lod", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, false, nullptr, frame,
                                          draw, dInstances, surf_tables_ok(dMaterials, numMaterials, dTextures, numTextures), drawIndex, width, height, band, dWorkspace,
                                          workspaceBytes, s))
        return st;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (draw->flags & SAILOR_SURFACE_GLTF) {
        sailor_launch(ctx, k_surface_visibility_lod_gltf, s.grid, dim3(256), s.P, s.V, *draw, reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials, dTextures,
                      numTextures, drawIndex, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
        SAILOR_CHECK_LAUNCH(ctx, "k_surface_visibility_lod_gltf");
    } else {
        sailor_launch(ctx, k_surface_visibility_lod, s.grid, dim3(256), s.P, s.V, *draw, reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials, dTextures,
                      numTextures, drawIndex, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
        SAILOR_CHECK_LAUNCH(ctx, "k_surface_visibility_lod");
    }
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_draw_indirect_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                                         const SailorDrawIndexedIndirectData* dCommand, const SailorPerInstanceData* dInstances, uint32_t numInstanceRecords,
                                         const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures,
                                         uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes)
{
    SurfDrawSetup s;
    if (const int st = surf_draw_prologue(ctx, "sailor_hip_surface_draw_indirect_lod", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, false,
                                          &dCommand, frame, draw, dInstances, surf_tables_ok(dMaterials, numMaterials, dTextures, numTextures), drawIndex, width, height, band,
                                          dWorkspace, workspaceBytes, s))
        return st;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* command = reinterpret_cast<const uint32_t*>(dCommand);
    if (draw->flags & SAILOR_SURFACE_GLTF) {
        sailor_launch(ctx, k_surface_visibility_indirect_lod_gltf, s.grid, dim3(256), s.P, s.V, *draw, command, numInstanceRecords, reinterpret_cast<const float*>(dInstances),
                      dMaterials, numMaterials, dTextures, numTextures, drawIndex, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
        SAILOR_CHECK_LAUNCH(ctx, "k_surface_visibility_indirect_lod_gltf");
    } else {
        sailor_launch(ctx, k_surface_visibility_indirect_lod, s.grid, dim3(256), s.P, s.V, *draw, command, numInstanceRecords, reinterpret_cast<const float*>(dInstances),
                      dMaterials, numMaterials, dTextures, numTextures, drawIndex, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
        SAILOR_CHECK_LAUNCH(ctx, "k_surface_visibility_indirect_lod");
    }
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_resolve_lod(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials,
                                   uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, int32_t width, int32_t height, const SailorBand* band,
                                   const void* dWorkspace, size_t workspaceBytes, float* dSurface, size_t planeStride, float* dDepthOutOrNull, uint8_t* dCoverageOrNull,
                                   const float* dAoInOrNull, float* dAoOutOrNull, float* dEmissive)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SurfResolveSetup s;
    const char* why = surf_resolve_why(frame, dInstances && surf_tables_ok(dMaterials, numMaterials, dTextures, numTextures), width, height, band, dWorkspace, workspaceBytes,
                                       dSurface, planeStride, dDepthOutOrNull, s);
    if (!why && ((dAoInOrNull && !aligned(dAoInOrNull, 4)) || (dAoOutOrNull && !aligned(dAoOutOrNull, 4)))) why = "an occlusion plane is misaligned";
    if (!why && !aligned(dEmissive, 16)) why = "the emissive plane is NULL or not 16-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_surface_resolve_lod", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_resolve_lod, texel_grid(width, band->fbRowCount), dim3(256), s.P, s.V, reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials,
                  dTextures, numTextures, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, s.maxDraws, dWorkspace, reinterpret_cast<float4*>(dSurface),
                  planeStride, dDepthOutOrNull, dCoverageOrNull, dAoInOrNull, dAoOutOrNull, reinterpret_cast<float4*>(dEmissive));
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_resolve_lod");
    return SAILOR_HIP_OK;
}

} // extern "C"
