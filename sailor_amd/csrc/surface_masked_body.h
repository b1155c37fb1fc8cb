// The draw kernel of the Masked queue as a body two translation units instantiate: surface_masked.hip (Standard.shader's ALPHA_CUTOUT: albedo[3] through
// albedoSampler against the constant 0.5) and surface_gltf.hip (Standard_glTF.shader's: baseColorFactor[3] through baseColorSampler against the material's
// alphaCutoff).  GLTF is a template argument, so each kernel holds its own record's offsets and, for Standard, no threshold word at all.
// LOD (default false: the kernels as they were) makes the alpha fetch the implicit-level-of-detail one of surface_lod.h: the lane also carries the level
// count of the albedo descriptor and the six steps of the edge functions to the next pixel, so a fragment can evaluate uv at its quad's other centres.
// MODE (default SURF_DRAW_MASKED, likewise) chooses what a fragment does: SURF_DRAW_PEEL is the Transparent queue's draw of surface_transparent.hip -- the same
// fragments against a read-only depth plane, keyed by order --, SURF_DRAW_BUCKET its one-rasterisation draw of surface_buckets.hip: the same fragments again,
// inserted into the pixel's K + 1 ordered slots.  SURF_DRAW_MSAA is the multisampled draw of surface_msaa.hip: the walk is surface_fill_msaa.h's over pixels, a
// fragment is a pixel with its covered samples, and the keys go to the per-sample store.
#pragma once
#include <type_traits>
#include "surface_fill.h"
#include "surface_fill_msaa.h"
#include "surface_lod.h"

// what the alpha of a fragment needs of its triangle, prepared once by the owning lane: the three clip w, (u, v, colour alpha) of the three set-up
// vertices -- the cut lerp aI + (aO - aI) t applied, in the order the winding swap left (SurfSrc's) --, the material's albedo[3] and the resolved albedo
// descriptor (texels == nullptr: no texels, the fetch is 0).  16 words and a pointer.  height < 0: a draw without ALPHA_CUTOUT, nothing is tested -- kept per lane
// in a vector register on purpose: as a wave-uniform flag it would hold a pair of scalar registers as a mask through all the loops, and the scalar file is full.
// cutoff: the material's alphaCutoff, read and carried by the glTF kernel only.
struct SurfAlpha { float w[3], u[3], v[3], c[3]; float albedoA; const uint32_t* texels; int width, height; float cutoff; };
// LOD: dx[k], dy[k] = what edge function k gains one pixel to the right / one row down (exact: the neighbour's edge functions are affine steps of the
// pixel's own); levels = the descriptor's level count n (1: today's fetch, no derivative)
struct SurfAlphaLod : SurfAlpha { long long dx[3], dy[3]; int levels; };
template <bool LOD> using SurfAlphaOf = std::conditional_t<LOD, SurfAlphaLod, SurfAlpha>;

// the part of SurfAlpha that belongs to the instance, not to the triangle's part: read once per lane BEFORE the loop over the parts, so that the two tables and
// their lengths are dead (and their scalar registers free) while the triangles are filled.  The table is one array of 80-byte slots; GLTF decides which record
// a slot is read as.
template <bool GLTF, bool LOD = false>
__device__ __forceinline__ void surf_alpha_material(SurfAlphaOf<LOD>& A, const float* __restrict__ model, const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
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
    if constexpr (LOD) A.levels = texels ? surf_level_count(d.width, d.height, d.levels) : 1;
}

// the steps of the three edge functions of a set-up triangle (surf_fill's dx, dy)
__device__ __forceinline__ void surf_alpha_steps(SurfAlphaLod& A, const SurfTri& t)
{
    A.dx[0] = -256ll * (t.y2 - t.y1); A.dx[1] = -256ll * (t.y0 - t.y2); A.dx[2] = -256ll * (t.y1 - t.y0);
    A.dy[0] = 256ll * (t.x2 - t.x1); A.dy[1] = 256ll * (t.x0 - t.x2); A.dy[2] = 256ll * (t.x1 - t.x0);
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

template <bool GLTF, bool LOD = false>
__device__ __forceinline__ SurfAlphaOf<LOD> surf_alpha_bcast(const SurfAlphaOf<LOD>& a, int src)
{
    SurfAlphaOf<LOD> b;
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
    if constexpr (LOD) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            b.dx[k] = surf_bcast64(a.dx[k], src); b.dy[k] = surf_bcast64(a.dy[k], src);
            SURF_KEEP_VECTOR(b.dx[k]); SURF_KEEP_VECTOR(b.dy[k]);
        }
        b.levels = __shfl(a.levels, src, 64);
        SURF_KEEP_VECTOR(b.levels);
    }
    return b;
}

// Standard.shader:383 + :403-408 at the pixel whose edge functions are e0, e1, e2: alpha = (mat.albedo[3] * tA.w) * a[8] in k_surface_resolve's operation
// order (the barycentrics and the three varyings by the header's formula), kept unless alpha < 0.5f -- a NaN alpha survives, as in GLSL.
// Standard_glTF.shader:389 + :410-415: the same alpha from baseColorFactor[3], kept unless alpha < alphaCutoff (a NaN on either side survives).
// LOD: tA.w is the implicit-level-of-detail fetch; (i, j) is the fragment's pixel, whose parity says where its quad's other centres lie.
template <bool GLTF, bool LOD = false>
__device__ __forceinline__ bool surf_alpha_keeps(const SurfAlphaOf<LOD>& A, int i, int j, long long e0, long long e1, long long e2, float area)
{
    if (A.height < 0) return true;
    const float l0 = (float)e0 / area, l1 = (float)e1 / area, l2 = (float)e2 / area;
    const float q0 = l0 / A.w[0], q1 = l1 / A.w[1], q2 = l2 / A.w[2];
    const float s = (q0 + q1) + q2;
    const float b0 = q0 / s, b1 = q1 / s, b2 = q2 / s;
    const float u = (A.u[0] * b0 + A.u[1] * b1) + A.u[2] * b2;
    const float v = (A.v[0] * b0 + A.v[1] * b1) + A.v[2] * b2;
    const float c = (A.c[0] * b0 + A.c[1] * b1) + A.c[2] * b2;
    float tA;
    if constexpr (LOD) {
        if (A.levels > 1) {
            float ux, vx, uy, vy;
            const bool left = (i & 1) != 0, up = (j & 1) != 0; // the row mate is to the left of an odd column, the column mate above an odd row
            surf_uv_at(A.u, A.v, A.w, e0 + (left ? -A.dx[0] : A.dx[0]), e1 + (left ? -A.dx[1] : A.dx[1]), e2 + (left ? -A.dx[2] : A.dx[2]), area, ux, vx);
            surf_uv_at(A.u, A.v, A.w, e0 + (up ? -A.dy[0] : A.dy[0]), e1 + (up ? -A.dy[1] : A.dy[1]), e2 + (up ? -A.dy[2] : A.dy[2]), area, uy, vy);
            tA = surf_texture_alpha_lod(A.texels, A.width, A.height, A.levels, u, v, surf_derivs(i, j, u, v, ux, vx, uy, vy));
        } else tA = surf_texture_alpha(A.texels, A.width, A.height, u, v);
    } else tA = surf_texture_alpha(A.texels, A.width, A.height, u, v);
    const float alpha = (A.albedoA * tA) * c;
    if constexpr (GLTF) return !(alpha < A.cutoff);
    else return !(alpha < 0.5f);
}

// surf_fragment with the discard between the plain load and the atomic: only a fragment whose key would win evaluates alpha, only a survivor issues the
// atomicMax.  (A stale load can only be smaller than what is stored: a fragment that would lose anyway may evaluate alpha in vain, never the reverse.)
template <bool GLTF, bool LOD = false>
__device__ __forceinline__ void surf_fragment_masked(unsigned long long* p, int i, int j, float z, unsigned int orderPlus1, const SurfAlphaOf<LOD>& A, long long e0,
                                                     long long e1, long long e2, float area)
{
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | orderPlus1;
    if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (surf_alpha_keeps<GLTF, LOD>(A, i, j, e0, e1, e2, area)) atomicMax(p, key);
    }
}

// PEEL (surface_transparent.hip, the Transparent queue): the depth attachment is read only and a pixel keeps, of the fragments beyond the order it committed
// last, the one of the SMALLEST order.  depth = the raw depth of the whole frame, last = the band's rows of the orders committed so far (0: none), both as
// uint32 words, both plain loads.  The key is (0xFFFFFFFF - orderPlus1) << 32 | zbits, so the maximum is the smallest order; it is issued as
// surf_fragment_masked issues its own: plain load, the discard only for a fragment that would win, then the atomicMax.
struct SurfPeel { const uint32_t* depth; const uint32_t* last; };
template <bool GLTF, bool LOD = false>
__device__ __forceinline__ void surf_fragment_peel(unsigned long long* p, const SurfPeel& peel, size_t atFrame, size_t atBand, int i, int j, float z, unsigned int orderPlus1,
                                                   const SurfAlphaOf<LOD>& A, long long e0, long long e1, long long e2, float area)
{
    const unsigned int zbits = __float_as_uint(z);
    if (zbits < peel.depth[atFrame]) return;    // GreaterOrEqual on the images of two non-negative floats: equal depth passes; nothing is written back
    if (orderPlus1 <= peel.last[atBand]) return; // blended by an earlier layer
    const unsigned long long key = ((unsigned long long)(0xFFFFFFFFu - orderPlus1) << 32) | zbits;
    if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (surf_alpha_keeps<GLTF, LOD>(A, i, j, e0, e1, e2, area)) atomicMax(p, key);
    }
}

// BUCKET (surface_buckets.hip, the Transparent queue in one rasterisation): a pixel keeps its first K fragments in primitive order, and whether there is a
// (K + 1)-th.  buckets = K + 1 planes of 64-bit slots over the band's rows, plane-major, `plane` slots apart; a slot holds orderPlus1 << 32 | zbits or
// SURF_BUCKET_EMPTY (all ones: never a key, an order that would reach 2^32 - 1 is refused by the entry point).  After the draws plane p holds the pixel's
// (p + 1)-th smallest key among the fragments that exist; plane K is the sentinel, non-empty exactly where the pixel has more than K fragments.
//
// The insertion is order-free and made of 64-bit atomicMin alone: a fragment with key v walks p = 0 .. K; old = atomicMin(&slot[p], v); old == EMPTY: the
// slot was free, stop; otherwise go on with max(old, v); what is carried past plane K is dropped.  Why every schedule leaves the same planes: plane 0 ends as
// the minimum of everything offered to it, whatever the arrival order.  Every other value offered to plane 0 is carried to plane 1 EXACTLY ONCE: as itself
// when it met something smaller (its atomicMin changed nothing and max(old, v) = v), or, when it was stored, by the one smaller value that later displaces it
// (that atomicMin returns it as `old`, and max(old, v) = old).  So plane 1 is offered everything but the minimum and ends as its minimum, the second
// smallest; and so on by induction down to plane K.  The keys of a pixel are distinct (a primitive has at most one fragment there), so no tie arises.
//
// Two shortcuts, both exact because a slot only ever decreases, so a relaxed load of it (surf_fragment_masked's idiom) can only show a value that is too LARGE:
//   - v > slot[p] as loaded proves the atomicMin there would store nothing and return something smaller than v: the walk goes to p + 1 with v, without it;
//   - v > slot[K] as loaded proves v is not among the pixel's K + 1 smallest (the slot is at or above its final value, the (K + 1)-th smallest of everything
//     that is inserted): the fragment is dropped with no atomic at all, and before its discard is evaluated.
// The order of a fragment's tests: depth, the plane-K reject, the discard, the chain -- a discarded fragment never touches a slot.
#define SURF_BUCKET_EMPTY 0xFFFFFFFFFFFFFFFFull
struct SurfBucket { const uint32_t* depth; unsigned long long* buckets; size_t plane; uint32_t layers; };
template <bool GLTF, bool LOD = false>
__device__ __forceinline__ void surf_fragment_bucket(const SurfBucket& b, size_t atFrame, size_t atBand, int i, int j, float z, unsigned int orderPlus1,
                                                     const SurfAlphaOf<LOD>& A, long long e0, long long e1, long long e2, float area)
{
    const unsigned int zbits = __float_as_uint(z);
    if (zbits < b.depth[atFrame]) return;   // surf_fragment_peel's test: equal depth passes, nothing is written back
    unsigned long long v = ((unsigned long long)orderPlus1 << 32) | zbits;
    unsigned long long* slot = b.buckets + atBand;
    if (v > __hip_atomic_load(slot + (size_t)b.layers * b.plane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // the pixel is full below this order
    if (!surf_alpha_keeps<GLTF, LOD>(A, i, j, e0, e1, e2, area)) return;
    for (uint32_t p = 0; p <= b.layers; p++, slot += b.plane) {
        if (v > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) continue;
        const unsigned long long old = atomicMin(slot, v);
        if (old == SURF_BUCKET_EMPTY) return;
        v = old > v ? old : v;
    }
}

// MSAA (surface_msaa.hip, the multisampled pass; the Multisampled section of include/sailor_hip.h has the rules): one fragment a pixel and primitive, one key a
// SAMPLE.  p = the pixel's S keys (pixel-major store).  The order of work is surf_fragment_masked's, per pixel: every sample that is covered (`full`: all of
// them, untested) and whose depth exists is compared with a plain relaxed load of its key; the discard is evaluated ONCE, with the edge functions of the pixel
// CENTRE (which may be negative: the barycentrics extrapolate), and only if some sample would win; only those samples issue the atomicMax.  The sample loop is
// kept a loop (the alpha words are live across it); a winner's depth is computed again behind the discard rather than kept for S samples.
struct SurfMsaa { unsigned long long* store; unsigned long long pattern; int samples; };
template <bool GLTF>
__device__ __forceinline__ void surf_pixel_msaa(unsigned long long* p, int S, unsigned long long pattern, const SurfTri& t, const SurfMsaaEdges& m, int tl, bool full, int i,
                                                int j, unsigned int orderPlus1, const SurfAlpha& A, long long e0, long long e1, long long e2, float area)
{
    unsigned int wins = 0;
#pragma unroll 1
    for (int s = 0; s < S; s++) {
        const int mx = surf_msaa_dx(pattern, s), my = surf_msaa_dy(pattern, s);
        const long long s1 = surf_msaa_at(m, 1, e1, mx, my), s2 = surf_msaa_at(m, 2, e2, mx, my);
        if (!full) {
            const long long s0 = surf_msaa_at(m, 0, e0, mx, my);
            if (s0 < 0 || s1 < 0 || s2 < 0) continue;
            if (surf_on_excluded_edge(s0, s1, s2, tl)) continue;
        }
        const float z = surf_depth(t, s1, s2, area);
        if (!(z > 0.0f && z <= 1.0f)) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | orderPlus1;
        if (key > __hip_atomic_load(p + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) wins |= 1u << s;
    }
    if (!wins) return;
    if (!surf_alpha_keeps<GLTF, false>(A, i, j, e0, e1, e2, area)) return;
#pragma unroll 1
    for (; wins; wins &= wins - 1u) {
        const int s = __builtin_ctz(wins);
        const int mx = surf_msaa_dx(pattern, s), my = surf_msaa_dy(pattern, s);
        const float z = surf_depth(t, surf_msaa_at(m, 1, e1, mx, my), surf_msaa_at(m, 2, e2, mx, my), area);
        atomicMax(p + s, ((unsigned long long)__float_as_uint(z) << 32) | orderPlus1);
    }
}

// what a draw kernel does with a fragment
enum { SURF_DRAW_MASKED = 0, SURF_DRAW_PEEL = 1, SURF_DRAW_BUCKET = 2 };
enum { SURF_DRAW_MSAA = 3 }; // (the multisampled pass: a fragment is a pixel with its covered samples)

// the slices (gridDim.y) are k_surface_visibility's; without SAILOR_SURFACE_ALPHA_CUTOUT in draw.flags the keys are k_surface_visibility's.
// X: what MODE needs beyond the workspace -- SurfPeel, SurfBucket under SURF_DRAW_BUCKET or SurfMsaa under SURF_DRAW_MSAA (the workspace then only takes the
// draw's descriptor).
template <bool GLTF, bool LOD = false, int MODE = SURF_DRAW_MASKED, typename X = SurfPeel>
__device__ __forceinline__ void surf_visibility_masked(const Mat4& P, const Mat4& V, const SailorSurfaceDraw& draw, const float* __restrict__ instances,
                                                       const SailorMaterialData* __restrict__ materials, uint32_t numMaterials,
                                                       const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t drawIndex, int W, int H,
                                                       int rowBegin, int rows, void* __restrict__ workspace, X peel = X())
{
    constexpr bool PEEL = MODE == SURF_DRAW_PEEL;
    const SurfWorkspace ws = surf_workspace(workspace, (size_t)rows * W);
    const unsigned int slice = blockIdx.y, slices = gridDim.y;
    if (blockIdx.x == 0 && slice == 0 && threadIdx.x == 0) ws.draws[drawIndex] = draw; // the resolve finds the draw here
    unsigned long long* keys = ws.keys;
    SURF_KEEP_VECTOR(keys); // (the last scalar pair that was spilled)
    // two more pairs the scalar file does not have.  The Standard peel keeps the compiler's allocation: 4 scalar spills to vector lanes at 168 registers, the
    // siblings' 3 waves per SIMD (pinned: none at 171, 2 waves).  The glTF peel has 2 waves either way (170 with the spills), so there they are pinned: 173, none.
    if constexpr (PEEL && GLTF) { SURF_KEEP_VECTOR(peel.depth); SURF_KEEP_VECTOR(peel.last); }
    // The bucket draws keep the compiler's allocation in both: 15 scalar spills to vector lanes (none read inside the insertion's walk) at 168 registers and 3
    // waves (Standard), 170 and 2 (glTF).  Pinning any of SurfBucket's words takes the Standard one to 170 or more, 2 waves; pinning all leaves 2 spills at 177 / 179.
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
    SurfAlphaOf<LOD> A;
    memset(&A, 0, sizeof A);
    A.height = -1;
    if (have && (draw.flags & SAILOR_SURFACE_ALPHA_CUTOUT)) surf_alpha_material<GLTF, LOD>( // (the entry point has checked that materials and textures are there)
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
            t = surface_setup<MODE == SURF_DRAW_MSAA>(P, V, model, vertices, draw.dIndices + 3 * (size_t)tri, Wl, H, rowB, rowE, (fl & (int)SAILOR_SURFACE_CULL_BACK) != 0, part,
                                                      second, S);
            if (A.height >= 0 && t.valid) {
                surf_alpha_vertices(A, S, vertices);
                if constexpr (LOD) surf_alpha_steps(A, t);
            }
        }
        const unsigned int orderPlus1 = draw.primBase + (unsigned int)(2ull * id) + (unsigned int)part + 1u; // (the entry point has checked the range)
        // the fill: the alpha words are the payload, carried to the wave once per large triangle
        if constexpr (MODE == SURF_DRAW_MSAA) {
            static_assert(!LOD, "the multisampled draw fetches the base level");
            surf_fill_msaa(t, orderPlus1, A, [](const SurfAlpha& a, int src) { return surf_alpha_bcast<GLTF, false>(a, src); }, slice, slices, lane, peel.samples, peel.pattern,
                           [&](int i, int j, const SurfTri& tri, const SurfMsaaEdges& m, int tl, bool full, unsigned int tag, const SurfAlpha& a, long long e0, long long e1,
                               long long e2, float area) {
                               surf_pixel_msaa<GLTF>(peel.store + ((size_t)(j - rowBegin) * W + i) * (size_t)peel.samples, peel.samples, peel.pattern, tri, m, tl, full, i, j, tag,
                                                     a, e0, e1, e2, area);
                           });
        } else {
            surf_fill(t, orderPlus1, A, [](const SurfAlphaOf<LOD>& a, int src) { return surf_alpha_bcast<GLTF, LOD>(a, src); }, slice, slices, lane,
                      [&](int i, int j, float z, unsigned int tag, const SurfAlphaOf<LOD>& a, long long e0, long long e1, long long e2, float area) {
                          if constexpr (MODE == SURF_DRAW_BUCKET) {
                              surf_fragment_bucket<GLTF, LOD>(peel, (size_t)j * W + i, (size_t)(j - rowBegin) * W + i, i, j, z, tag, a, e0, e1, e2, area);
                          } else if constexpr (PEEL) {
                              const size_t atBand = (size_t)(j - rowBegin) * W + i;
                              surf_fragment_peel<GLTF, LOD>(keys + atBand, peel, (size_t)j * W + i, atBand, i, j, z, tag, a, e0, e1, e2, area);
                          } else surf_fragment_masked<GLTF, LOD>(keys + (size_t)(j - rowBegin) * W + i, i, j, z, tag, a, e0, e1, e2, area);
                      });
        }
        if (part == 0) again = second;
    }
}

// the command of an indirect draw, read where the draw runs (surface_indirect.hip, surface_lod.hip).  Rule 3 of the indirect section:
// n = min(instanceCount, capacity, numInstanceRecords - firstInstance), 0 when firstInstance >= numInstanceRecords
__device__ __forceinline__ bool surf_indirect_command(SailorSurfaceDraw& draw, const uint32_t* __restrict__ command, uint32_t numInstanceRecords)
{
    const uint32_t count = command[1], first = command[4]; // SailorDrawIndexedIndirectData.instanceCount, .firstInstance: uniform addresses, plain loads
    const uint32_t room = first < numInstanceRecords ? numInstanceRecords - first : 0u;
    uint32_t n = count < draw.numDrawn ? count : draw.numDrawn; // (numDrawn arrives as the capacity)
    n = n < room ? n : room;
    draw.numDrawn = n;
    draw.firstInstance = first;
    // block 0 stays for the descriptor, whatever the count
    return blockIdx.x == 0 || (unsigned long long)blockIdx.x * 256ull < (unsigned long long)n * draw.numTriangles;
}
