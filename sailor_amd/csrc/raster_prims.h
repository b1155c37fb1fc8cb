// The rasterisers' primitives, written once for raster.hip (the shadow maps and the depth prepass) and the surface pass (surface_common.h), so that a
// fragment's depth is the prepass's bit for bit: the set-up triangle, the exact 64-bit edge function, the top-left rule, the floor division of the
// 1/256-pixel grid, the near-plane cut and the 64-bit lane broadcast.  oracle/sailor_oracle.c (oracle_raster_depth) has the pinned rules.
#pragma once
#include "common.h"
#include <math.h>

struct SurfTri { long long x0, y0, x1, y1, x2, y2; float z0, z1, z2; int i0, i1, j0, j1; bool valid; };

__device__ __forceinline__ long long surf_floor_div256(long long a) { return a >= 0 ? a / 256 : -((-a + 255) / 256); }
// A vertex beyond the near plane of the reversed depth range (z_clip > w_clip, which includes everything behind the eye) cannot be projected:
// such a triangle is cut against w - z = 0 in clip space first.  The new vertex on an edge is always computed from its inside end,
// P = I + (O - I) * t with t = dI / (dI - dO) and d = w - z, one rounding per operation.  One vertex inside (A; B, C follow it in the triangle's
// own order): the triangle (A, AB, AC).  Two inside (A, B; C outside follows them): the quad A, B, BC, AC as the triangles
// (A, B, BC) = part 0 and (A, BC, AC) = part 1.  Triangles wholly inside are untouched (their fragments beyond the plane fail z <= 1).
__device__ __forceinline__ float4 surf_cut(const float4& I, float dI, const float4& O, float dO, float& t)
{
    t = dI / (dI - dO);
    return make_float4(I.x + (O.x - I.x) * t, I.y + (O.y - I.y) * t, I.z + (O.z - I.z) * t, I.w + (O.w - I.w) * t);
}
__device__ __forceinline__ long long surf_edge(long long ax, long long ay, long long bx, long long by, long long px, long long py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
__device__ __forceinline__ bool surf_top_left(long long ax, long long ay, long long bx, long long by)
{
    const long long dx = bx - ax, dy = by - ay;
    return (dy == 0 && dx > 0) || dy < 0;
}
__device__ __forceinline__ long long surf_bcast64(long long v, int src)
{
    const int lo = __shfl((int)(unsigned int)(unsigned long long)v, src, 64), hi = __shfl((int)((unsigned long long)v >> 32), src, 64);
    return (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo);
}
