// What the passes with one texel per lane share: 256-thread blocks of 64 x 4 texels, so that a wave's texels are contiguous in x, and the checks
// their entry points make before the first launch.  The predicates that combine these checks stay with their entry points.
#pragma once
#include "common.h"

#define TEXEL_MAX_EXTENT 32768

// texel (texel_i(), texel_j()) of the calling lane under a grid of texel_grid(w, h) and a block of 256
__device__ __forceinline__ int texel_i() { return (int)(blockIdx.x * 64 + (threadIdx.x & 63)); }
__device__ __forceinline__ int texel_j() { return (int)(blockIdx.y * 4 + (threadIdx.x >> 6)); }

static dim3 texel_grid(int32_t w, int32_t h) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)); }
static bool extent_ok(int32_t w, int32_t h) { return w > 0 && h > 0 && w <= TEXEL_MAX_EXTENT && h <= TEXEL_MAX_EXTENT; }
// non-NULL and a multiple of `bytes`, a power of two
static bool aligned(const void* p, size_t bytes) { return p && ((uintptr_t)p & (bytes - 1)) == 0; }
static bool overlaps(const void* a, size_t aBytes, const void* b, size_t bBytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bBytes && b0 < a0 + aBytes;
}
