// The implicit level of detail of texture() in the surface pass (include/sailor_hip.h, "Mip-mapped material textures"): the level count of a descriptor, where
// a level begins, the scale factor of a pixel from its quad's fine derivatives, the two levels and their weight, and the trilinear fetch.  Everything is a pure
// function of (the owning primitive's set-up, the pixel): the derivatives come from the exact integer edge functions at the centres of the pixel's 2 x 2 quad,
// inside the triangle or not, so no lane reads another lane's result.  tests/lod_ref.py restates it sequentially; the kernels are held to it bit for bit.
#pragma once
#include "surface_common.h"
#include "canonical_math.h"

// floor(log2(max(width, height))) + 1 in integers (TextureImporter.cpp:247-295); width, height >= 1
static __host__ __device__ __forceinline__ int surf_full_levels(int width, int height)
{
    int m = width > height ? width : height, n = 0;
    while (m > 0) { n++; m >>= 1; }
    return n;
}
// n = clamp(levels, 1, full): 0 reads as 1
static __host__ __device__ __forceinline__ int surf_level_count(int width, int height, uint32_t levels)
{
    const int full = surf_full_levels(width, height);
    return levels < 1u ? 1 : (levels > (uint32_t)full ? full : (int)levels);
}
static __host__ __device__ __forceinline__ int surf_level_extent(int extent, int l) { return (extent >> l) > 1 ? (extent >> l) : 1; }
// sailor_hip_mip_chain_texels(width, height, l)
static __host__ __device__ __forceinline__ size_t surf_level_offset(int width, int height, int l)
{
    size_t n = 0;
    for (int k = 0; k < l; k++) n += (size_t)surf_level_extent(width, k) * (size_t)surf_level_extent(height, k);
    return n;
}

// uv of the set-up triangle at the pixel centre whose edge functions are e0, e1, e2: a[0], a[1] of the header's varying formula over the three vertices'
// (cut-lerped) texcoords U, V and clip w
__device__ __forceinline__ void surf_uv_at(const float U[3], const float V[3], const float w[3], long long e0, long long e1, long long e2, float area, float& u, float& v)
{
    const float l0 = (float)e0 / area, l1 = (float)e1 / area, l2 = (float)e2 / area;
    const float q0 = l0 / w[0], q1 = l1 / w[1], q2 = l2 / w[2];
    const float s = (q0 + q1) + q2;
    const float b0 = q0 / s, b1 = q1 / s, b2 = q2 / s;
    u = (U[0] * b0 + U[1] * b1) + U[2] * b2;
    v = (V[0] * b0 + V[1] * b1) + V[2] * b2;
}

// the fine derivatives of the quad at (i & ~1, j & ~1), seen from pixel (i, j): d/dx = uv(i | 1, j) - uv(i & ~1, j), d/dy = uv(i, j | 1) - uv(i, j & ~1).
// (u, v) is the pixel's own uv, (ux, vx) its row mate's (i ^ 1, j), (uy, vy) its column mate's (i, j ^ 1).
struct SurfDerivs { float dudx, dvdx, dudy, dvdy; };
__device__ __forceinline__ SurfDerivs surf_derivs(int i, int j, float u, float v, float ux, float vx, float uy, float vy)
{
    SurfDerivs d;
    d.dudx = (i & 1) ? u - ux : ux - u; d.dvdx = (i & 1) ? v - vx : vx - v;
    d.dudy = (j & 1) ? u - uy : uy - u; d.dvdy = (j & 1) ? v - vy : vy - v;
    return d;
}

// the level selection of a descriptor of n levels: level `hi` alone (blend == false) or t_hi (1 - delta) + t_lo delta with lo = hi + 1
struct SurfLod { int hi; float delta; bool blend; };
__device__ __forceinline__ SurfLod surf_lod_select(int width, int height, int n, const SurfDerivs& d)
{
    SurfLod L;
    L.hi = 0; L.delta = 0.0f; L.blend = false;
    if (n <= 1) return L;
    const float fw = (float)width, fh = (float)height;
    const float ax = d.dudx * fw, bx = d.dvdx * fh, ay = d.dudy * fw, by = d.dvdy * fh;
    const float rx = ax * ax + bx * bx, ry = ay * ay + by * by;
    const float r2 = ry > rx ? ry : rx;
    if (!(r2 > 1.0f)) return L;                             // magnification, zero, NaN
    L.hi = n - 1;
    if (r2 >= ldexpf(1.0f, 2 * (n - 1))) return L;          // 4^(n-1) and beyond, +inf
    const float lambda = 0.5f * canonical_log2f(r2);
    const int hi = (int)lambda;
    if (hi >= n - 1) return L;
    L.hi = hi; L.delta = lambda - (float)hi; L.blend = true;
    return L;
}

// texture(textureSamplers[index], uv) at the implicit level of detail: trilinear, each level the base-level fetch over that level's extents
__device__ __forceinline__ float4 surf_texture_lod(const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t index, const float* __restrict__ srgb,
                                                   float u, float v, const SurfDerivs& dv)
{
    const SailorTextureDesc d = textures[index < numTextures ? index : 0u];
    if (!d.texels || d.width <= 0 || d.height <= 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const SurfLod L = surf_lod_select(d.width, d.height, surf_level_count(d.width, d.height, d.levels), dv);
    const int wh = surf_level_extent(d.width, L.hi), hh = surf_level_extent(d.height, L.hi);
    const uint32_t* __restrict__ level = d.texels + surf_level_offset(d.width, d.height, L.hi);
    const float4 a = surf_texels_fetch(level, wh, hh, d.flags, srgb, u, v);
    if (!L.blend) return a;
    const int lo = L.hi + 1; // (level lo begins where level hi ends)
    const float4 b = surf_texels_fetch(level + (size_t)wh * (size_t)hh, surf_level_extent(d.width, lo), surf_level_extent(d.height, lo), d.flags, srgb, u, v);
    const float k = 1.0f - L.delta;
    return make_float4(a.x * k + b.x * L.delta, a.y * k + b.y * L.delta, a.z * k + b.z * L.delta, a.w * k + b.w * L.delta);
}

// the alpha of that fetch alone (surf_texture_alpha per level); texels == nullptr: no texels, 0
__device__ __forceinline__ float surf_texture_alpha_lod(const uint32_t* __restrict__ texels, int width, int height, int n, float u, float v, const SurfDerivs& dv)
{
    if (!texels || width <= 0 || height <= 0) return 0.0f;
    const SurfLod L = surf_lod_select(width, height, n, dv);
    const int wh = surf_level_extent(width, L.hi), hh = surf_level_extent(height, L.hi);
    const uint32_t* __restrict__ level = texels + surf_level_offset(width, height, L.hi);
    const float a = surf_texture_alpha(level, wh, hh, u, v);
    if (!L.blend) return a;
    const int lo = L.hi + 1;
    const float b = surf_texture_alpha(level + (size_t)wh * (size_t)hh, surf_level_extent(width, lo), surf_level_extent(height, lo), u, v);
    return a * (1.0f - L.delta) + b * L.delta;
}
