// glTF materials in the surface pass: Standard_glTF.shader, the shader ModelImporter.cpp:156-231 gives every imported model, where it differs from
// Standard.shader -- the normal matrix of the tangent basis (:136-138), the material record (:42-58), the orm / occlusion / emissive fetches (:389-396), the
// emissive term (:399) and alphaCutoff (:411).  include/sailor_hip.h has the pinned rules; tests/gltf_ref.py restates them sequentially and the kernels are
// held to it bit for bit.  The shade kernels are not touched: the resolve here produces their inputs and the composite adds the emissive term behind them.
//
//   k_surface_visibility_gltf  surface_masked_body.h's draw, instantiated for the glTF record: baseColorFactor[3] through baseColorSampler against the
//                              material's alphaCutoff.  Without ALPHA_CUTOUT the keys are k_surface_visibility's.
//   k_surface_resolve_gltf     k_surface_resolve for a pass that mixes both shaders: the owning draw's flag picks the record a material slot is read as, the
//                              matrix under the tangent basis (mat3(model) or its inverse transpose) and the fetches.  A pixel of a Standard draw computes
//                              exactly k_surface_resolve's operations.  Next to the three planes it writes the emissive plane and the occlusion the shade
//                              is to read (min(g_AO, occlusion texel)).  The fetches are consumed one at a time, so no more than one is live next to the varyings.
//   k_surface_composite_gltf   target = covered ? (emissive.rgb + radiance.rgb, radiance.a) : target
#include "surface_masked_body.h"

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
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    const size_t at = (size_t)jb * W + i;
    const unsigned long long key = ws.keys[at];
    const unsigned int low = (unsigned int)key;
    if (depthOut) depthOut[at] = __uint_as_float((unsigned int)(key >> 32));
    float4 p0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p1 = make_float4(0.0f, 0.0f, 1.0f, 1.0f), p2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 em = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    float ao = aoIn ? aoIn[at] : 1.0f; // (aoOut may be aoIn itself: this lane's word is read before it is written, and by no other lane)
    bool covered = false;
    if (low != 0u) {
        const unsigned int order = low - 1u;
        // the last descriptor whose primBase does not exceed the order (empty slots hold 0xFFFFFFFF)
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
                const long long px = 256ll * i + 128, py = 256ll * (jb + rowBegin) + 128;
                const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
                const float l0 = (float)surf_edge(t.x1, t.y1, t.x2, t.y2, px, py) / area, l1 = (float)surf_edge(t.x2, t.y2, t.x0, t.y0, px, py) / area,
                            l2 = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, px, py) / area;
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
                float a[18]; // (statically indexed under full unrolling: registers)
#pragma unroll
                for (int c = 0; c < 18; c++) {
                    const float a0 = surf_varying_basis(vI0, model, n, c); // (vertex 0 is never a cut one)
                    float a1 = surf_varying_basis(vI1, model, n, c), a2 = surf_varying_basis(vI2, model, n, c);
                    if (S.cut[1]) a1 = a1 + (surf_varying_basis(vO1, model, n, c) - a1) * S.t[1];
                    if (S.cut[2]) a2 = a2 + (surf_varying_basis(vO2, model, n, c) - a2) * S.t[2];
                    a[c] = (a0 * b0 + a1 * b1) + a2 * b2;
                }
                const uint32_t mi = reinterpret_cast<const uint32_t*>(model)[20]; // PerInstanceData.materialInstance, flat
                // one 80-byte slot, read as the record of the owning draw: words (floats / uints) of SailorMaterialData or of SailorGltfMaterialData
                const SailorMaterialData* __restrict__ sm = materials + (mi < numMaterials ? mi : 0u);
                const SailorGltfMaterialData* __restrict__ gm = reinterpret_cast<const SailorGltfMaterialData*>(sm);
                const float u = a[0], v = a[1];
                // :383 / glTF :389 -- albedo and baseColorFactor both sit at offset 0
                {
                    const float4 tA = surf_texture(textures, numTextures, gltf ? gm->baseColorSampler : sm->albedoSampler, ws.srgb, u, v);
                    p2.x = (sm->albedo[0] * tA.x) * a[5]; p2.y = (sm->albedo[1] * tA.y) * a[6]; p2.z = (sm->albedo[2] * tA.z) * a[7];
                    p0 = make_float4(a[2], a[3], a[4], (sm->albedo[3] * tA.w) * a[8]);
                }
                // :384-385 (.x of two samplers) / glTF :390-391 (.z and .y of ONE fetch)
                {
                    const float4 tO = surf_texture(textures, numTextures, gltf ? gm->ormSampler : sm->metalnessSampler, ws.srgb, u, v);
                    if (gltf) {
                        p2.w = gm->metallicFactor * tO.z;
                        p1.w = gm->roughnessFactor * tO.y;
                    } else {
                        p2.w = sm->metallic * tO.x;
                        p1.w = sm->roughness * surf_texture(textures, numTextures, sm->roughnessSampler, ws.srgb, u, v).x;
                    }
                }
                if (gltf) {
                    // :392 min(g_AO, occlusion texel) = y < x ? y : x; :393, :399 the emissive term
                    const float tOcc = surf_texture(textures, numTextures, gm->occlusionSampler, ws.srgb, u, v).x;
                    const float4 tE = surf_texture(textures, numTextures, gm->emissiveSampler, ws.srgb, u, v);
                    em = make_float4(gm->emissiveFactor[0] * tE.x, gm->emissiveFactor[1] * tE.y, gm->emissiveFactor[2] * tE.z, tOcc);
                    ao = (tOcc < ao) ? tOcc : ao;
                }
                // :388-389 / glTF :395-396
                const float4 tN = surf_texture(textures, numTextures, gltf ? gm->normalSampler : sm->normalSampler, ws.srgb, u, v);
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
    SurfDrawSetup s;
    if (const int st = surf_draw_prologue(ctx, "sailor_hip_surface_draw_gltf", SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF, true, nullptr, frame,
                                          draw, dInstances, surf_tables_ok(dMaterials, numMaterials, dTextures, numTextures), drawIndex, width, height, band, dWorkspace,
                                          workspaceBytes, s))
        return st;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_visibility_gltf, s.grid, dim3(256), s.P, s.V, *draw, reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials, dTextures,
                  numTextures, drawIndex, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_visibility_gltf");
    return SAILOR_HIP_OK;
}

int sailor_hip_surface_resolve_gltf(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials,
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
    if (why) return surf_refuse(ctx, "sailor_hip_surface_resolve_gltf", why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_surface_resolve_gltf, texel_grid(width, band->fbRowCount), dim3(256), s.P, s.V, reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials,
                  dTextures, numTextures, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, s.maxDraws, dWorkspace, reinterpret_cast<float4*>(dSurface),
                  planeStride, dDepthOutOrNull, dCoverageOrNull, dAoInOrNull, dAoOutOrNull, reinterpret_cast<float4*>(dEmissive));
    SAILOR_CHECK_LAUNCH(ctx, "k_surface_resolve_gltf");
    return SAILOR_HIP_OK;
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
