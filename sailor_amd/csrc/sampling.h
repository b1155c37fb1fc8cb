// Canonical texture sampling, the only place of the library that turns a coordinate into tap indices.  For shade.hip (K3 shadow lookups, ambient / IBL
// term) and ibl_prefilter.hip: manual bilinear taps (texel centres at (i + 0.5) / size, clamp-to-edge), the Vulkan cube face table (ties z over y over x)
// and the cube mip chain layout -- level-major, then face, then size x size float4 texels.  Must match oracle/sailor_oracle.c bit for bit.
// For the post-process passes (hbao.hip, post_tail.hip, bloom.hip, sky.hip, sky_clouds.hip): Repeat addressing, byte texels and whole-plane samples.
// Non-finite coordinates (a NaN normal, an infinite roughness; a hardware sampler's result for them is undefined, so the choice is this path's own):
// the (int) conversions below are the device's saturating convert -- NaN -> 0, +-inf -> INT_MAX / INT_MIN -- every tap index is clamped into the
// image AFTER the conversion and without an addition that could wrap (see bilinear_taps: a roughness of +inf once read the BRDF table at row INT_MIN),
// so no fetch leaves it, and the weights (inf - inf) are NaN, so the sample is NaN.  The oracle's conversion is defined to
// give the same (sat_int / tap_pair there; plain (int)x is undefined in C for such values); tests/test_ambient_gpu.py compares these pixels by class.
// Two conversions, on purpose.  bilinear_taps keeps the plain (int): it is the shade's hot path, its coordinates come from normals and roughness, which
// are finite for every sane input, and v_cvt_i32_f32 is what the cast compiles to.  bilinear_taps_saturating spells the same conversion out
// (cvt_i32_saturating) for the passes whose coordinates are computed from the depth buffer -- HBAO's ray march, motion blur's reprojection -- where one
// hostile texel (0, inf, NaN) makes them non-finite as a matter of course: there nothing is left to what a compiler makes of an undefined cast.  The float
// arithmetic and, wherever the cast is defined, the taps of the two are the same.
#pragma once
#include "common.h"
#include <limits.h>

struct BilinearTaps { int x0, x1, y0, y1; float ax, ay; };

__device__ __forceinline__ BilinearTaps bilinear_taps(int W, int H, float u, float v)
{
    BilinearTaps t;
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    t.ax = x - fx; t.ay = y - fy;
    // the second tap as clamp(x0, -1, W - 2) + 1, not clamp(x0 + 1, 0, W - 1): the same index for every x0, but x0 = INT_MAX (a +inf coordinate) cannot wrap --
    // the compiler turns the other form into max(x0, -1) + 1 BEFORE the upper clamp, and INT_MAX + 1 = INT_MIN then passes min(., W - 1) as a negative index
    const int x0 = (int)fx, y0 = (int)fy;
    t.x0 = min(max(x0, 0), W - 1); t.x1 = min(max(x0, -1), W - 2) + 1;
    t.y0 = min(max(y0, 0), H - 1); t.y1 = min(max(y0, -1), H - 2) + 1;
    return t;
}

__device__ __forceinline__ float lerp2(float t00, float t10, float t01, float t11, float ax, float ay)
{
    const float top = t00 * (1.0f - ax) + t10 * ax;
    const float bot = t01 * (1.0f - ax) + t11 * ax;
    return top * (1.0f - ay) + bot * ay;
}

__device__ __forceinline__ void cube_face_st(float rx, float ry, float rz, int& face, float& s, float& t)
{
    const float ax = fabsf(rx), ay = fabsf(ry), az = fabsf(rz);
    float sc, tc, ma;
    if (az >= ax && az >= ay) { face = rz < 0.0f ? 5 : 4; sc = rz < 0.0f ? -rx : rx; tc = -ry; ma = az; }
    else if (ay >= ax)        { face = ry < 0.0f ? 3 : 2; sc = rx; tc = ry < 0.0f ? -rz : rz; ma = ay; }
    else                      { face = rx < 0.0f ? 1 : 0; sc = rx < 0.0f ? rz : -rz; tc = -ry; ma = ax; }
    s = 0.5f * (sc / ma + 1.0f);
    t = 0.5f * (tc / ma + 1.0f);
}

__device__ __forceinline__ float4 bilinear_f4(const float4* __restrict__ tex, int size, float s, float t)
{
    const BilinearTaps b = bilinear_taps(size, size, s, t);
    const float4 a = tex[(size_t)b.y0 * size + b.x0], c = tex[(size_t)b.y0 * size + b.x1];
    const float4 d = tex[(size_t)b.y1 * size + b.x0], e = tex[(size_t)b.y1 * size + b.x1];
    return make_float4(lerp2(a.x, c.x, d.x, e.x, b.ax, b.ay), lerp2(a.y, c.y, d.y, e.y, b.ax, b.ay),
                       lerp2(a.z, c.z, d.z, e.z, b.ax, b.ay), lerp2(a.w, c.w, d.w, e.w, b.ax, b.ay));
}

__device__ __forceinline__ float4 cube_sample_level(const float4* __restrict__ cube, int size0, int level, int face, float s, float t)
{
    size_t off = 0;
    for (int l = 0; l < level; l++) { const int sz = max(size0 >> l, 1); off += (size_t)6 * sz * sz; }
    const int size = max(size0 >> level, 1);
    return bilinear_f4(cube + off + (size_t)face * size * size, size, s, t);
}

__device__ __forceinline__ float4 cube_sample_lod(const float4* __restrict__ cube, int size0, int levels, float rx, float ry, float rz, float lod)
{
    int face; float s, t;
    cube_face_st(rx, ry, rz, face, s, t);
    const float maxLod = (float)(levels - 1);
    lod = lod < 0.0f ? 0.0f : (lod > maxLod ? maxLod : lod);
    const float fl = floorf(lod);
    const int l0 = (int)fl, l1 = min(l0 + 1, levels - 1);
    const float f = lod - fl;
    const float4 a = cube_sample_level(cube, size0, l0, face, s, t), b = cube_sample_level(cube, size0, l1, face, s, t);
    return make_float4(a.x * (1.0f - f) + b.x * f, a.y * (1.0f - f) + b.y * f, a.z * (1.0f - f) + b.z * f, a.w * (1.0f - f) + b.w * f);
}

// ---- Repeat addressing and byte texels: the cloud march's weather map and noise volumes, the sky and dirt planes ---------------------------------
// A tap index is wrapped into [0, n) AFTER the saturating conversion: i % n lies in (-n, n), so neither the + n nor the + 1 of the second tap can
// wrap an int, whatever the coordinate was (NaN -> 0, +-inf -> INT_MAX / INT_MIN).  The weights of a non-finite coordinate are NaN, the sample NaN.
__device__ __forceinline__ int wrap_tap(int i, int n) { return ((i % n) + n) % n; }
__device__ __forceinline__ int wrap_next(int i0, int n) { return i0 + 1 == n ? 0 : i0 + 1; }
__device__ __forceinline__ float unorm8(uint32_t byte) { return (float)byte / 255.0f; }

struct RepeatTap { int i0, i1; float a; };
__device__ __forceinline__ RepeatTap repeat_tap(int n, float u)
{
    RepeatTap t;
    const float x = u * (float)n - 0.5f, fx = floorf(x);
    t.a = x - fx;
    t.i0 = wrap_tap((int)fx, n);
    t.i1 = wrap_next(t.i0, n);
    return t;
}

// sampler3D over an n^3 R8_UNORM volume, x fastest, base level, trilinear, Repeat: the x pairs first, then y (lerp2), then z
__device__ __forceinline__ float trilinear_repeat_r8(const uint8_t* __restrict__ vol, int n, float u, float v, float w)
{
    const RepeatTap X = repeat_tap(n, u), Y = repeat_tap(n, v), Z = repeat_tap(n, w);
    const uint8_t* __restrict__ z0 = vol + (size_t)Z.i0 * n * n;
    const uint8_t* __restrict__ z1 = vol + (size_t)Z.i1 * n * n;
    const int r0 = Y.i0 * n, r1 = Y.i1 * n;
    const float lo = lerp2(unorm8(z0[r0 + X.i0]), unorm8(z0[r0 + X.i1]), unorm8(z0[r1 + X.i0]), unorm8(z0[r1 + X.i1]), X.a, Y.a);
    const float hi = lerp2(unorm8(z1[r0 + X.i0]), unorm8(z1[r0 + X.i1]), unorm8(z1[r1 + X.i0]), unorm8(z1[r1 + X.i1]), X.a, Y.a);
    return lo * (1.0f - Z.a) + hi * Z.a;
}

// sampler2D over a W x H RGBA8 image (one uint32 per texel, r in the low byte), bilinear, Repeat
__device__ __forceinline__ float4 bilinear_repeat_rgba8(const uint32_t* __restrict__ tex, int W, int H, float u, float v)
{
    const RepeatTap X = repeat_tap(W, u), Y = repeat_tap(H, v);
    const uint32_t a = tex[Y.i0 * W + X.i0], c = tex[Y.i0 * W + X.i1], d = tex[Y.i1 * W + X.i0], e = tex[Y.i1 * W + X.i1];
    float4 r;
    r.x = lerp2(unorm8(a & 255u), unorm8(c & 255u), unorm8(d & 255u), unorm8(e & 255u), X.a, Y.a);
    r.y = lerp2(unorm8((a >> 8) & 255u), unorm8((c >> 8) & 255u), unorm8((d >> 8) & 255u), unorm8((e >> 8) & 255u), X.a, Y.a);
    r.z = lerp2(unorm8((a >> 16) & 255u), unorm8((c >> 16) & 255u), unorm8((d >> 16) & 255u), unorm8((e >> 16) & 255u), X.a, Y.a);
    r.w = lerp2(unorm8(a >> 24), unorm8(c >> 24), unorm8(d >> 24), unorm8(e >> 24), X.a, Y.a);
    return r;
}

// nearest tap of a Repeat sampler: texel floor(u * n) mod n
__device__ __forceinline__ int nearest_repeat(int n, float u) { return wrap_tap((int)floorf(u * (float)n), n); }
// nearest tap of a clamp-to-edge sampler
__device__ __forceinline__ int nearest_clamp(int n, float u) { return min(max((int)floorf(u * (float)n), 0), n - 1); }

// ---- Whole planes: the samplers of the post-process passes -----------------------------------------------------------------------------------------
// float -> int as v_cvt_i32_f32 defines it: NaN -> 0, saturating at the ends of int32
__device__ __forceinline__ int cvt_i32_saturating(float x)
{
    if (x != x) return 0;
    if (x >= 2147483648.0f) return INT_MAX;
    if (x <= -2147483648.0f) return INT_MIN;
    return (int)x;
}

// bilinear_taps (the same float arithmetic, the same taps wherever its cast is defined) with the conversion above; the clamp runs before the + 1, so no
// integer overflows either
__device__ __forceinline__ BilinearTaps bilinear_taps_saturating(int W, int H, float u, float v)
{
    BilinearTaps t;
    const float x = u * (float)W - 0.5f, y = v * (float)H - 0.5f;
    const float fx = floorf(x), fy = floorf(y);
    t.ax = x - fx; t.ay = y - fy;
    const int x0 = min(max(cvt_i32_saturating(fx), -1), W - 1), y0 = min(max(cvt_i32_saturating(fy), -1), H - 1);
    t.x0 = max(x0, 0); t.x1 = min(x0 + 1, W - 1);
    t.y0 = max(y0, 0); t.y1 = min(y0 + 1, H - 1);
    return t;
}

// sampler2D over a W x H float plane, bilinear, clamp-to-edge, the saturating taps
__device__ __forceinline__ float sample_clamp_f1(const float* __restrict__ p, int W, int H, float u, float v)
{
    const BilinearTaps t = bilinear_taps_saturating(W, H, u, v);
    const float* __restrict__ r0 = p + (size_t)t.y0 * (size_t)W;
    const float* __restrict__ r1 = p + (size_t)t.y1 * (size_t)W;
    return lerp2(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.ax, t.ay);
}

// the four taps of a W-wide float4 plane, all four channels
__device__ __forceinline__ float4 lerp2_f4(const float4* __restrict__ p, int W, const BilinearTaps t)
{
    const float4* __restrict__ r0 = p + (size_t)t.y0 * (size_t)W;
    const float4* __restrict__ r1 = p + (size_t)t.y1 * (size_t)W;
    const float4 a = r0[t.x0], c = r0[t.x1], d = r1[t.x0], e = r1[t.x1];
    return make_float4(lerp2(a.x, c.x, d.x, e.x, t.ax, t.ay), lerp2(a.y, c.y, d.y, e.y, t.ax, t.ay), lerp2(a.z, c.z, d.z, e.z, t.ax, t.ay),
                       lerp2(a.w, c.w, d.w, e.w, t.ax, t.ay));
}
// sampler2D over a W x H float4 plane, bilinear: clamp-to-edge with either tap computation, and Repeat
__device__ __forceinline__ float4 sample_clamp_f4(const float4* __restrict__ p, int W, int H, float u, float v)
{
    return lerp2_f4(p, W, bilinear_taps(W, H, u, v));
}
__device__ __forceinline__ float4 sample_clamp_f4_saturating(const float4* __restrict__ p, int W, int H, float u, float v)
{
    return lerp2_f4(p, W, bilinear_taps_saturating(W, H, u, v));
}
__device__ __forceinline__ float4 sample_repeat_f4(const float4* __restrict__ p, int W, int H, float u, float v)
{
    const RepeatTap X = repeat_tap(W, u), Y = repeat_tap(H, v);
    return lerp2_f4(p, W, {X.i0, X.i1, Y.i0, Y.i1, X.a, Y.a});
}
