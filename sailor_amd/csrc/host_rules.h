// Host-side rules that more than one translation unit applies, in plain C++ (no HIP): a stand-alone program can include this file and
// cull_plan.h and check them without a device (scripts/cull_plan_host_check.cpp).  common.h includes it.
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>

#include "../../include/sailor_hip.h"

#define TILE SAILOR_LIGHTS_CULLING_TILE_SIZE
#define CAND SAILOR_LIGHTS_CANDIDATES_PER_TILE
#define KEEP SAILOR_LIGHTS_PER_TILE

// "A large light set": from here on a band of a split frame selects its own lights before the cull chain (light_cull.hip: plan_cull), a large band
// keeps the whole frame's shade form (cull_plan.h: band_takes_band_form) and every band's shade leaves wave slots to the cull chain (shade.hip: reserve).
#define LARGE_LIGHT_SET 131072

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- the band rule: the only place that turns (height, tile rows) into framebuffer rows ----
static inline void band_from_rows(int32_t height, int32_t r0, int32_t r1, SailorBand* b)
{
    b->tileRowBegin = r0;
    b->tileRowEnd = r1;
    // tile row t covers framebuffer rows H-1-16t-15 .. H-1-16t, clamped to [0, H)
    int32_t lo = height - TILE * r1;
    int32_t hi = height - TILE * r0;
    if (lo < 0) lo = 0;
    if (hi > height) hi = height;
    if (hi < lo) hi = lo;
    b->fbRowBegin = lo;
    b->fbRowCount = hi - lo;
}
static inline int32_t tile_rows_of(int32_t height) { return (height - 1) / TILE + 1; } // FrameGraph/LightCullingNode.cpp:57
// valid: the tile rows lie inside the frame and the band equals what band_from_rows gives for them (height > 0)
static inline bool band_is_valid(int32_t height, const SailorBand* b)
{
    if (!b || b->tileRowBegin < 0 || b->tileRowEnd > tile_rows_of(height) || b->tileRowBegin > b->tileRowEnd) return false;
    SailorBand want;
    band_from_rows(height, b->tileRowBegin, b->tileRowEnd, &want);
    return b->fbRowBegin == want.fbRowBegin && b->fbRowCount == want.fbRowCount;
}
// A null band means the whole frame (built in *whole); a band that is not valid for the frame gives null: the caller refuses.  (height > 0)
static inline const SailorBand* band_or_whole_frame(int32_t height, const SailorBand* band, SailorBand* whole)
{
    if (!band) { band_from_rows(height, 0, tile_rows_of(height), whole); return whole; }
    return band_is_valid(height, band) ? band : nullptr;
}

// ---- the shade's plane addressing ----
// The shade kernels address a pixel of the band's three surface planes and of the radiance plane by ONE 32-bit byte offset per lane on top of a scalar
// base (shade_body.h: !WIDE).  That holds while the last byte of a plane of the band lies below 2^32 -- 16 bytes a pixel: fbRowCount x width <= 2^28 pixels --
// and, as the planes' bases are derived one from the other in scalars, while the plane stride in bytes does too.  Anything larger takes the kernels with
// 64-bit pixel indices.  (width, fbRowCount > 0)
static inline bool shade_planes_fit_32_bits(size_t planeStridePixels, int32_t fbRowCount, int32_t width)
{
    const uint64_t limit = (uint64_t)1 << 28; // pixels of 16 bytes in 4 GB
    return (uint64_t)planeStridePixels < limit && (uint64_t)fbRowCount * (uint64_t)width <= limit;
}

// ---- integer A / B knobs from the environment ----
// Read once (`static const EnvKnob k = env_knob_read("NAME");` where it is used).  env_knob gives the value if it is set and inside [lo, hi], else -1:
// the default holds, and a value that was set but lies outside says so in *lastError (when there is a message and somewhere to put it).
struct EnvKnob { bool set; int raw; };
static inline EnvKnob env_knob_read(const char* name)
{
    const char* e = getenv(name);
    return EnvKnob { e != nullptr, e ? atoi(e) : -1 };
}
static inline int env_knob(const EnvKnob& k, long lo, long hi, std::string* lastError, const char* outOfRange)
{
    if (k.set && k.raw >= lo && k.raw <= hi) return k.raw;
    if (k.set && lastError && outOfRange) *lastError = outOfRange;
    return -1;
}
