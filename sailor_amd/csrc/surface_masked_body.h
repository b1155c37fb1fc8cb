// The draw kernel of the Masked queue as a body two translation units instantiate: surface_masked.hip (Standard.shader's ALPHA_CUTOUT: albedo[3] through
// albedoSampler against the constant 0.5) and surface_gltf.hip (Standard_glTF.shader's: baseColorFactor[3] through baseColorSampler against the material's
// alphaCutoff).  GLTF is a template argument, so each kernel holds its own record's offsets and, for Standard, no threshold word at all.
#pragma once
#include "surface_common.h"

// keeps a (wave-uniform or boolean) value in a vector register: the scalar file of the draw kernel is full (two matrices, the draw, the loops' masks)
#define SURF_KEEP_VECTOR(x) asm volatile("" : "+v"(x))

// what the alpha of a fragment needs of its triangle, prepared once by the owning lane: the three clip w, (u, v, colour alpha) of the three set-up
// vertices -- the cut lerp aI + (aO - aI) t applied, in the order the winding swap left (SurfSrc's) --, the material's albedo[3] and the resolved albedo
// descriptor (texels == nullptr: no texels, the fetch is 0).  16 words and a pointer.  height < 0: a draw without ALPHA_CUTOUT, nothing is tested -- kept per lane
// in a vector register on purpose: as a wave-uniform flag it would hold a pair of scalar registers as a mask through all the loops, and the scalar file is full.
// cutoff: the material's alphaCutoff, read and carried by the glTF kernel only.
struct SurfAlpha { float w[3], u[3], v[3], c[3]; float albedoA; const uint32_t* texels; int width, height; float cutoff; };

// the part of SurfAlpha that belongs to the instance, not to the triangle's part: read once per lane BEFORE the loop over the parts, so that the two tables and
// their lengths are dead (and their scalar registers free) while the triangles are filled.  The table is one array of 80-byte slots; GLTF decides which record
// a slot is read as.
template <bool GLTF>
__device__ __forceinline__ void surf_alpha_material(SurfAlpha& A, const float* __restrict__ model, const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                    const SailorTextureDesc* __restrict__ textures, uint32_t numTextures)
{
    const uint32_t mi = reinterpret_cast<const uint32_t*>(model)[20]; // PerInstanceData.materialInstance, flat
    const SailorMaterialData* __restrict__ mat = materials + (mi < numMaterials ? mi : 0u);
    uint32_t index;
    if constexpr (GLTF) {
        const SailorGltfMaterialData* __restrict__ g = reinterpret_cast<const SailorGltfMaterialData*>(mat);
        A.albedoA = g->baseColorFactor[3];
        A.cutoff = g->alphaCutoff;
        index = g->baseColorSampler;
    } else {
        A.albedoA = mat->albedo[3];
        index = mat->albedoSampler;
    }
    const SailorTextureDesc d = textures[index < numTextures ? index : 0u];
    const bool texels = d.texels && d.width > 0 && d.height > 0;
    A.texels = texels ? d.texels : nullptr; A.width = texels ? d.width : 0; A.height = texels ? d.height : 0;
}

__device__ __forceinline__ void surf_alpha_vertices(SurfAlpha& A, const SurfSrc& S, const float* __restrict__ vertices)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float* __restrict__ vI = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[k];
        float u = vI[0], v = vI[1], c = vI[17]; // surf_varying's 0, 1 and 8
        if (S.cut[k]) {
            const float* __restrict__ vO = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[k];
            u = u + (vO[0] - u) * S.t[k]; v = v + (vO[1] - v) * S.t[k]; c = c + (vO[17] - c) * S.t[k];
        }
        A.u[k] = u; A.v[k] = v; A.c[k] = c; A.w[k] = S.w[k];
    }
}

template <bool GLTF>
__device__ __forceinline__ SurfAlpha surf_alpha_bcast(const SurfAlpha& a, int src)
{
    SurfAlpha b;
#pragma unroll
    for (int k = 0; k < 3; k++) { b.w[k] = __shfl(a.w[k], src, 64); b.u[k] = __shfl(a.u[k], src, 64); b.v[k] = __shfl(a.v[k], src, 64); b.c[k] = __shfl(a.c[k], src, 64); }
    b.albedoA = __shfl(a.albedoA, src, 64);
    b.texels = reinterpret_cast<const uint32_t*>(surf_bcast64((long long)reinterpret_cast<uintptr_t>(a.texels), src));
    b.width = __shfl(a.width, src, 64); b.height = __shfl(a.height, src, 64);
    b.cutoff = 0.0f;
    if constexpr (GLTF) b.cutoff = __shfl(a.cutoff, src, 64);
    // the words are wave-uniform, and the compiler may move them to scalar registers next to the two matrices, the draw and the loops' masks, which fill the
    // scalar file already (DESIGN.md has what was spilled and why).  They are read by a few fragments only, so they stay in vector registers.
#pragma unroll
    for (int k = 0; k < 3; k++) { SURF_KEEP_VECTOR(b.w[k]); SURF_KEEP_VECTOR(b.u[k]); SURF_KEEP_VECTOR(b.v[k]); SURF_KEEP_VECTOR(b.c[k]); }
    SURF_KEEP_VECTOR(b.albedoA); SURF_KEEP_VECTOR(b.texels); SURF_KEEP_VECTOR(b.width); SURF_KEEP_VECTOR(b.height);
    if constexpr (GLTF) SURF_KEEP_VECTOR(b.cutoff);
    return b;
}

// Standard.shader:383 + :403-408 at the pixel whose edge functions are e0, e1, e2: alpha = (mat.albedo[3] * tA.w) * a[8] in k_surface_resolve's operation
// order (the barycentrics and the three varyings by the header's formula), kept unless alpha < 0.5f -- a NaN alpha survives, as in GLSL.
// Standard_glTF.shader:389 + :410-415: the same alpha from baseColorFactor[3], kept unless alpha < alphaCutoff (a NaN on either side survives).
template <bool GLTF>
__device__ __forceinline__ bool surf_alpha_keeps(const SurfAlpha& A, long long e0, long long e1, long long e2, float area)
{
    if (A.height < 0) return true;
    const float l0 = (float)e0 / area, l1 = (float)e1 / area, l2 = (float)e2 / area;
    const float q0 = l0 / A.w[0], q1 = l1 / A.w[1], q2 = l2 / A.w[2];
    const float s = (q0 + q1) + q2;
    const float b0 = q0 / s, b1 = q1 / s, b2 = q2 / s;
    const float u = (A.u[0] * b0 + A.u[1] * b1) + A.u[2] * b2;
    const float v = (A.v[0] * b0 + A.v[1] * b1) + A.v[2] * b2;
    const float c = (A.c[0] * b0 + A.c[1] * b1) + A.c[2] * b2;
    const float alpha = (A.albedoA * surf_texture_alpha(A.texels, A.width, A.height, u, v)) * c;
    if constexpr (GLTF) return !(alpha < A.cutoff);
    else return !(alpha < 0.5f);
}

// surf_fragment with the discard between the plain load and the atomic: only a fragment whose key would win evaluates alpha, only a survivor issues the
// atomicMax.  (A stale load can only be smaller than what is stored: a fragment that would lose anyway may evaluate alpha in vain, never the reverse.)
template <bool GLTF>
__device__ __forceinline__ void surf_fragment_masked(unsigned long long* p, float z, unsigned int orderPlus1, const SurfAlpha& A, long long e0, long long e1,
                                                     long long e2, float area)
{
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | orderPlus1;
    if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (surf_alpha_keeps<GLTF>(A, e0, e1, e2, area)) atomicMax(p, key);
    }
}

// the slices (gridDim.y) are k_surface_visibility's; without SAILOR_SURFACE_ALPHA_CUTOUT in draw.flags the keys are k_surface_visibility's
template <bool GLTF>
__device__ __forceinline__ void surf_visibility_masked(const Mat4& P, const Mat4& V, const SailorSurfaceDraw& draw, const float* __restrict__ instances,
                                                       const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                       const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                       int rowBegin, int rows, void* __restrict__ workspace)
{
    const SurfWorkspace ws = surf_workspace(workspace, (size_t)rows * W);
    const unsigned int slice = blockIdx.y, slices = gridDim.y;
    if (blockIdx.x == 0 && slice == 0 && threadIdx.x == 0) ws.draws[drawIndex] = draw; // the resolve finds the draw here
    unsigned long long* keys = ws.keys;
    SURF_KEEP_VECTOR(keys); // (the last scalar pair that was spilled)
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
    SurfAlpha A;
    memset(&A, 0, sizeof A);
    A.height = -1;
    if (have && (draw.flags & SAILOR_SURFACE_ALPHA_CUTOUT)) surf_alpha_material<GLTF>( // (the entry point has checked that materials and textures are there)
        A, instances + SURF_INSTANCE_FLOATS * (size_t)inst, materials, numMaterials, textures, numTextures);
    bool again = false;
    for (int part = 0; part < 2; part++) {
        if (part && !__any(again)) break;
        SurfTri t;
        t.valid = false;
        bool second = false;
        if (have && (part == 0 || again)) {
            SurfSrc S;
            const float* __restrict__ model = instances + SURF_INSTANCE_FLOATS * (size_t)inst;
            // the frame's extent and the flags go through an opaque scalar copy here: otherwise the compiler hoists the 64-bit forms of W - 1, rowBegin and
            // rowEnd - 1 and the cull mask out of all loops, and these eight scalar registers are the ones the file does not have (they were spilled)
            int Wl = W, rowB = rowBegin, rowE = rowBegin + rows, fl = (int)draw.flags;
            asm volatile("" : "+s"(Wl), "+s"(rowB), "+s"(rowE), "+s"(fl));
            t = surface_setup(P, V, model, vertices, draw.dIndices + 3 * (size_t)tri, Wl, H, rowB, rowE, (fl & (int)SAILOR_SURFACE_CULL_BACK) != 0, part, second, S);
            if (A.height >= 0 && t.valid) surf_alpha_vertices(A, S, vertices);
        }
        const unsigned int orderPlus1 = draw.primBase + (unsigned int)(2ull * id) + (unsigned int)part + 1u; // (the entry point has checked the range)
        const bool small = t.valid && (long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) <= SURF_SMALL_BOX;
        if (small && slice == 0) {
            const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
            // (the three top-left flags as bits of one vector register: as three booleans they are three scalar pairs through the loops, see SurfAlpha)
            int tl = (surf_top_left(t.x1, t.y1, t.x2, t.y2) ? 1 : 0) | (surf_top_left(t.x2, t.y2, t.x0, t.y0) ? 2 : 0) | (surf_top_left(t.x0, t.y0, t.x1, t.y1) ? 4 : 0);
            SURF_KEEP_VECTOR(tl);
            const long long px0 = 256ll * t.i0 + 128, py0 = 256ll * t.j0 + 128;
            long long r0 = surf_edge(t.x1, t.y1, t.x2, t.y2, px0, py0), r1 = surf_edge(t.x2, t.y2, t.x0, t.y0, px0, py0), r2 = surf_edge(t.x0, t.y0, t.x1, t.y1, px0, py0);
            const long long dx0 = -256ll * (t.y2 - t.y1), dx1 = -256ll * (t.y0 - t.y2), dx2 = -256ll * (t.y1 - t.y0);
            const long long dy0 = 256ll * (t.x2 - t.x1), dy1 = 256ll * (t.x0 - t.x2), dy2 = 256ll * (t.x1 - t.x0);
            for (int j = t.j0; j <= t.j1; j++, r0 += dy0, r1 += dy1, r2 += dy2) {
                long long e0 = r0, e1 = r1, e2 = r2;
                for (int i = t.i0; i <= t.i1; i++, e0 += dx0, e1 += dx1, e2 += dx2) {
                    if (e0 < 0 || e1 < 0 || e2 < 0) continue;
                    if ((e0 == 0 && !(tl & 1)) || (e1 == 0 && !(tl & 2)) || (e2 == 0 && !(tl & 4))) continue;
                    const float z = (t.z0 + (t.z1 - t.z0) * ((float)e1 / area)) + (t.z2 - t.z0) * ((float)e2 / area);
                    if (z > 0.0f && z <= 1.0f) surf_fragment_masked<GLTF>(keys + (size_t)(j - rowBegin) * W + i, z, orderPlus1, A, e0, e1, e2, area);
                }
            }
        }
        // the large ones: the whole wave on one triangle at a time; the alpha words travel with the geometry
        unsigned long long todo = __ballot(t.valid && !small);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            SurfTri b;
            b.x0 = surf_bcast64(t.x0, src); b.y0 = surf_bcast64(t.y0, src); b.x1 = surf_bcast64(t.x1, src); b.y1 = surf_bcast64(t.y1, src);
            b.x2 = surf_bcast64(t.x2, src); b.y2 = surf_bcast64(t.y2, src);
            b.z0 = __shfl(t.z0, src, 64); b.z1 = __shfl(t.z1, src, 64); b.z2 = __shfl(t.z2, src, 64);
            b.i0 = __shfl(t.i0, src, 64); b.i1 = __shfl(t.i1, src, 64); b.j0 = __shfl(t.j0, src, 64); b.j1 = __shfl(t.j1, src, 64);
            const unsigned int bOrder = (unsigned int)__shfl((int)orderPlus1, src, 64);
            const SurfAlpha B = surf_alpha_bcast<GLTF>(A, src);
            const float area = (float)surf_edge(b.x0, b.y0, b.x1, b.y1, b.x2, b.y2);
            int tl = (surf_top_left(b.x1, b.y1, b.x2, b.y2) ? 1 : 0) | (surf_top_left(b.x2, b.y2, b.x0, b.y0) ? 2 : 0) | (surf_top_left(b.x0, b.y0, b.x1, b.y1) ? 4 : 0);
            SURF_KEEP_VECTOR(tl);
            unsigned int number = 0;
            for (int sj = b.j0 >> 6; sj <= (b.j1 >> 6); sj++)
                for (int si = b.i0 >> 6; si <= (b.i1 >> 6); si++) {
                    if (number++ % slices != slice) continue;
                    const int bi = si * 8 + (lane & 7), bj = sj * 8 + (lane >> 3);
                    bool alive = bi >= (b.i0 >> 3) && bi <= (b.i1 >> 3) && bj >= (b.j0 >> 3) && bj <= (b.j1 >> 3);
                    if (alive) {
                        long long m0 = -0x7FFFFFFFFFFFFFFFll, m1 = m0, m2 = m0;
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            const long long px = 256ll * (bi * 8 + ((c & 1) ? 7 : 0)) + 128, py = 256ll * (bj * 8 + ((c & 2) ? 7 : 0)) + 128;
                            m0 = max(m0, surf_edge(b.x1, b.y1, b.x2, b.y2, px, py)); m1 = max(m1, surf_edge(b.x2, b.y2, b.x0, b.y0, px, py));
                            m2 = max(m2, surf_edge(b.x0, b.y0, b.x1, b.y1, px, py));
                        }
                        alive = m0 >= 0 && m1 >= 0 && m2 >= 0;
                    }
                    unsigned long long live = __ballot(alive);
                    while (live) { // the surviving blocks, one lane per texel
                        const int s2 = __builtin_ctzll(live);
                        live &= live - 1ull;
                        const int i = (si * 8 + (s2 & 7)) * 8 + (lane & 7), j = (sj * 8 + (s2 >> 3)) * 8 + (lane >> 3);
                        if (i >= b.i0 && i <= b.i1 && j >= b.j0 && j <= b.j1) {
                            const long long px = 256ll * i + 128, py = 256ll * j + 128;
                            const long long e0 = surf_edge(b.x1, b.y1, b.x2, b.y2, px, py), e1 = surf_edge(b.x2, b.y2, b.x0, b.y0, px, py),
                                            e2 = surf_edge(b.x0, b.y0, b.x1, b.y1, px, py);
                            const bool in = !(e0 < 0 || e1 < 0 || e2 < 0) && !((e0 == 0 && !(tl & 1)) || (e1 == 0 && !(tl & 2)) || (e2 == 0 && !(tl & 4)));
                            if (in) {
                                const float z = (b.z0 + (b.z1 - b.z0) * ((float)e1 / area)) + (b.z2 - b.z0) * ((float)e2 / area);
                                if (z > 0.0f && z <= 1.0f) surf_fragment_masked<GLTF>(keys + (size_t)(j - rowBegin) * W + i, z, bOrder, B, e0, e1, e2, area);
                            }
                        }
                    }
                }
        }
        if (part == 0) again = second;
    }
}
