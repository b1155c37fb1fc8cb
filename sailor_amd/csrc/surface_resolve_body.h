// The resolve of the surface pass as ONE body three kernels instantiate, and the search that finds a pixel's draw:
//
//   k_surface_resolve       (surface.hip)      surf_resolve_pixel<false, false>: Standard.shader alone, three planes
//   k_surface_resolve_gltf  (surface_gltf.hip) surf_resolve_pixel<true, false>: a pass that mixes Standard.shader and Standard_glTF.shader; the emissive and
//                                              occlusion planes next to the three
//   k_surface_resolve_lod   (surface_lod.hip)  surf_resolve_pixel<true, true>: the same with every fetch at its implicit level of detail
//
// A lane per pixel: key -> draw (surf_owning_draw) -> instance, triangle, part; the set-up again, the edge functions at this pixel, the varyings one by one
// (never all 54 vertex values at once), the material slot, the fetches -- consumed one at a time, so no more than one is live next to the varyings.
// MIXED and LOD are template arguments: what a kernel does not do is not in its code, and what two kernels both do is the same written operations in the
// same order, one fp32 rounding each (the library is built without contraction).  That is what makes a pixel of a Standard draw the same bits through all
// three, and a table of one-level descriptors the same bits with and without LOD; the GPU tests hold both.
#pragma once
#include "surface_masked_body.h"

// The draw an order belongs to: the last descriptor whose primBase does not exceed the order (a binary search; empty slots hold 0xFFFFFFFF; maxDraws from the
// workspace's size, as begin derived it), then d = the instance's running number in the draw and r = 2 * triangle + part.  False: no live draw holds the order.
__device__ __forceinline__ bool surf_owning_draw(const SurfWorkspace& ws, uint32_t maxDraws, unsigned int order, SailorSurfaceDraw& draw, unsigned int& d, unsigned int& r)
{
    unsigned int lo = 0, hi = maxDraws;
    while (hi - lo > 1u) {
        const unsigned int mid = lo + ((hi - lo) >> 1);
        if (ws.draws[mid].primBase <= order) lo = mid; else hi = mid;
    }
    draw = ws.draws[lo];
    const unsigned int rel = order - draw.primBase;
    const unsigned int per = 2u * draw.numTriangles;
    d = per ? rel / per : 0xFFFFFFFFu;
    r = rel - d * per;
    return draw.primBase <= order && d < draw.numDrawn;
}

// MIXED = false: every draw is Standard.shader's, and aoIn, aoOut and emissive are not read, written or looked at.
// The line numbers are Standard.shader's, those after "glTF" Standard_glTF.shader's.
template <bool MIXED, bool LOD>
__device__ __forceinline__ void surf_resolve_pixel(const Mat4& P, const Mat4& V, const float* __restrict__ instances, const SailorMaterialData* __restrict__ materials,
                                                   uint32_t numMaterials, const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, int W, int H, int rowBegin,
                                                   int rows, uint32_t maxDraws, const void* __restrict__ workspace, float4* __restrict__ surface, size_t planeStride,
                                                   float* __restrict__ depthOut, uint8_t* __restrict__ coverage, const float* aoIn, float* aoOut, float4* __restrict__ emissive)
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
    float ao = 1.0f;
    if constexpr (MIXED) ao = aoIn ? aoIn[at] : 1.0f; // (aoOut may be aoIn itself: this lane's word is read before it is written, and by no other lane)
    bool covered = false;
    SailorSurfaceDraw draw;
    unsigned int d, r;
    if (low != 0u && surf_owning_draw(ws, maxDraws, low - 1u, draw, d, r)) {
        const unsigned int tri = r >> 1;
        const int part = (int)(r & 1u);
        const bool gltf = MIXED && (draw.flags & SAILOR_SURFACE_GLTF) != 0; // the owning draw's flag picks the record, the matrix under the basis and the fetches
        const uint32_t inst = draw.dInstanceIds ? draw.dInstanceIds[d] : draw.firstInstance + d;
        const float* __restrict__ model = instances + SURF_INSTANCE_FLOATS * (size_t)inst;
        const float* __restrict__ vertices = reinterpret_cast<const float*>(draw.dVertices);
        bool second;
        SurfSrc S;
        const SurfTri t = surface_setup(P, V, model, vertices, draw.dIndices + 3 * (size_t)tri, W, H, rowBegin, rowBegin + rows, (draw.flags & SAILOR_SURFACE_CULL_BACK) != 0,
                                        part, second, S);
        if (t.valid) {
            covered = true;
            const int j = jb + rowBegin;
            const long long px = 256ll * i + 128, py = 256ll * j + 128;
            const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
            const long long e0 = surf_edge(t.x1, t.y1, t.x2, t.y2, px, py), e1 = surf_edge(t.x2, t.y2, t.x0, t.y0, px, py), e2 = surf_edge(t.x0, t.y0, t.x1, t.y1, px, py);
            const float l0 = (float)e0 / area, l1 = (float)e1 / area, l2 = (float)e2 / area;
            const float q0 = l0 / S.w[0], q1 = l1 / S.w[1], q2 = l2 / S.w[2];
            const float s = (q0 + q1) + q2;
            const float b0 = q0 / s, b1 = q1 / s, b2 = q2 / s;
            const float* __restrict__ vI0 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[0];
            const float* __restrict__ vI1 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[1];
            const float* __restrict__ vI2 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[2];
            const float* __restrict__ vO1 = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[1];
            const float* __restrict__ vO2 = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[2];
            float n[9]; // :138 mat3(model), glTF :136-138 its inverse transpose: under a copy of mat3(model) surf_varying_basis is surf_varying
            surf_basis_matrix(model, gltf, n);
            float a[18]; // (statically indexed under full unrolling: registers)
            float U[3], Vv[3]; // LOD: the three set-up vertices' texcoords, the cut lerp applied: what uv at the quad's other centres needs
#pragma unroll
            for (int c = 0; c < 18; c++) {
                const float a0 = surf_varying_basis(vI0, model, n, c); // (vertex 0 is never a cut one)
                float a1 = surf_varying_basis(vI1, model, n, c), a2 = surf_varying_basis(vI2, model, n, c);
                if (S.cut[1]) a1 = a1 + (surf_varying_basis(vO1, model, n, c) - a1) * S.t[1];
                if (S.cut[2]) a2 = a2 + (surf_varying_basis(vO2, model, n, c) - a2) * S.t[2];
                if constexpr (LOD) {
                    if (c == 0) { U[0] = a0; U[1] = a1; U[2] = a2; }
                    if (c == 1) { Vv[0] = a0; Vv[1] = a1; Vv[2] = a2; }
                }
                a[c] = (a0 * b0 + a1 * b1) + a2 * b2;
            }
            const float u = a[0], v = a[1];
            SurfDerivs dv;
            if constexpr (LOD) {
                // rule 3 of the mip-mapped section: uv at the row mate (i ^ 1, j) and the column mate (i, j ^ 1), inside the triangle and the frame or not
                const long long mx = 256ll * (i ^ 1) + 128, my = 256ll * (j ^ 1) + 128;
                float ux, vx, uy, vy;
                surf_uv_at(U, Vv, S.w, surf_edge(t.x1, t.y1, t.x2, t.y2, mx, py), surf_edge(t.x2, t.y2, t.x0, t.y0, mx, py), surf_edge(t.x0, t.y0, t.x1, t.y1, mx, py), area,
                           ux, vx);
                surf_uv_at(U, Vv, S.w, surf_edge(t.x1, t.y1, t.x2, t.y2, px, my), surf_edge(t.x2, t.y2, t.x0, t.y0, px, my), surf_edge(t.x0, t.y0, t.x1, t.y1, px, my), area,
                           uy, vy);
                dv = surf_derivs(i, j, u, v, ux, vx, uy, vy);
            }
            // texture(textureSamplers[index], uv): the base level, or -- LOD -- the implicit level of detail
            const auto tex = [&](uint32_t index) {
                if constexpr (LOD) return surf_texture_lod(textures, numTextures, index, ws.srgb, u, v, dv);
                else return surf_texture(textures, numTextures, index, ws.srgb, u, v);
            };
            const uint32_t mi = reinterpret_cast<const uint32_t*>(model)[20]; // PerInstanceData.materialInstance, flat
            // one 80-byte slot, read as the record of the owning draw: words (floats / uints) of SailorMaterialData or of SailorGltfMaterialData
            const SailorMaterialData* __restrict__ sm = materials + (mi < numMaterials ? mi : 0u);
            const SailorGltfMaterialData* __restrict__ gm = reinterpret_cast<const SailorGltfMaterialData*>(sm);
            // :383 / glTF :389 -- albedo and baseColorFactor both sit at offset 0
            {
                const float4 tA = tex(gltf ? gm->baseColorSampler : sm->albedoSampler);
                p2.x = (sm->albedo[0] * tA.x) * a[5]; p2.y = (sm->albedo[1] * tA.y) * a[6]; p2.z = (sm->albedo[2] * tA.z) * a[7];
                p0 = make_float4(a[2], a[3], a[4], (sm->albedo[3] * tA.w) * a[8]);
            }
            // :384-385 (.x of two samplers) / glTF :390-391 (.z and .y of ONE fetch)
            {
                const float4 tO = tex(gltf ? gm->ormSampler : sm->metalnessSampler);
                if (gltf) {
                    p2.w = gm->metallicFactor * tO.z;
                    p1.w = gm->roughnessFactor * tO.y;
                } else {
                    p2.w = sm->metallic * tO.x;
                    p1.w = sm->roughness * tex(sm->roughnessSampler).x;
                }
            }
            if (gltf) {
                // glTF :392 min(g_AO, occlusion texel) = y < x ? y : x; :393, :399 the emissive term
                const float tOcc = tex(gm->occlusionSampler).x;
                const float4 tE = tex(gm->emissiveSampler);
                em = make_float4(gm->emissiveFactor[0] * tE.x, gm->emissiveFactor[1] * tE.y, gm->emissiveFactor[2] * tE.z, tOcc);
                ao = (tOcc < ao) ? tOcc : ao;
            }
            // :388-389 / glTF :395-396
            const float4 tN = tex(gltf ? gm->normalSampler : sm->normalSampler);
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
    surface[at] = p0;
    surface[planeStride + at] = p1;
    surface[2 * planeStride + at] = p2;
    if constexpr (MIXED) {
        emissive[at] = em;
        if (aoOut) aoOut[at] = ao;
    }
    if (coverage) coverage[at] = covered ? 1 : 0;
}
