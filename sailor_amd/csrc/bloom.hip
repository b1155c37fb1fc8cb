// Bloom for gfx950: the Bloom node, the one node between the two RenderScene passes and EyeAdaptation that rewrites `Main` in place
// (tests/golden/DefaultRenderer.renderer:296-304).
//
// Replaces the 2 (levels - 1) Dispatches recorded by BloomNode::Process (FrameGraph/BloomNode.cpp:21-144):
//   * Content/Shaders/ComputeBloomDownscale.shader:72-127, level i -> i + 1 (BloomNode.cpp:99-116)  -> k_bloom_downscale
//   * Content/Shaders/ComputeBloomUpscale.shader:44-95, level i -> i - 1, i = levels - 1 .. 1 (:122-141) -> k_bloom_upscale
// The levels of `Main` are RGBA32F planes of one level-major chain, row 0 = top, level l = max(1, width >> l) x max(1, height >> l).
// Named divergence: the reference's images are rgba16f; nothing is rounded through half here (as for Sky and the shade's radiance).
//
// Arithmetic is evaluated exactly as the shaders write it, in their order, one IEEE rounding per operation (-ffp-contract=off, IEEE division, denormals
// kept); tests/bloom_ref.py restates it in NumPy float32 and the kernels reproduce it bit for bit.  Where GLSL fixes no order this file uses the
// library's: dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, vec4 / float = one division per component, sums and products left to right, every literal
// is its fp32 value (div = (1 / 4) * (0.5, 0.125) = (0.125, 0.03125)).
//
// Decisions where "as written" needs one:
//   * Source texels.  Both shaders fill a 10 x 10 tile per 8 x 8 group: slot i reads
//         ivec2(readDim * ((vec2(8 g - 1) + 0.5) * (1.0 / writeDim) + vec2(i % 10, i / 10) * (1.0 / writeDim)))
//     in fp32, and the truncation is toward zero.  That is NOT "texel 2 p + 1": for 2160 -> 1080 rows 828 of the 3 240 in-range (row, neighbour) taps
//     resolve to 2 p, and the same absolute neighbour can resolve to different rows for two groups.  So output pixel x with neighbour d in {-1, 0, 1}
//     takes its index from base = 8 (x >> 3) - 1 and slot = (x & 7) + 1 + d, per axis (bloom_src_index), whatever the block shape is; nothing is
//     shared between lanes, so nothing needs the indices of two lanes to agree.
//   * An imageLoad outside the image is undefined in the reference without robust image access: (0, 0, 0, 0) here.  In the downscale that is the
//     one column / row in front of texel 0 and the ones behind readDim - 1; in the upscale the lower halo (about -0.25) truncates to texel 0 and
//     only the upper halo (readDim) is outside.  Stores outside writeDim are dropped.
//   * load_lds returns alpha 1 (the tile keeps r, g, b only): the downscale writes the sum of its five Karis weights into alpha, the upscale adds
//     bloomIntensity (16 / 16 of it), and the dirt term, to the destination's alpha.
//   * u_threshold is the node's (BloomNode.cpp:93): (t, t - knee, 2 knee, 0.25 knee) -- .w is a product where the shader's comment expects a quotient.
//     Restated, not repaired (sailor_host_bloom_push_constants).
//   * max is glsl_max of common.h; clamp(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x): a NaN passes through clamp.
//   * texture(u_dirt_texture, uv) (u_mip_level == 1 only): four-tap fp32 bilinear with Repeat addressing, no mips
//     (Content/Textures/Bokeh__Lens_Dirt_9.jpg.asset), over the caller's decoded linear float4 texels -- sample_repeat_f4 of sampling.h.
//     A NULL dirt plane means "no dirt term": an extension for hosts without the asset.
//
// Shape.  One output texel per lane, a float4 (16 B) each, 256-thread blocks of 64 x 4 texels so that a wave's rows are contiguous in x.  The nine
// taps are nine independent float4 loads: a source texel is asked for by up to nine lanes of neighbouring rows of the same block, which the vector
// cache serves; the tile, its LDS round trip and its barrier are gone.  The downscale touches every second source row and half of every line of
// those rows; the upscale streams the destination once in, once out.  The small levels are one launch each (launch-latency bound; not folded).
#include "common.h"
#include "sampling.h"
#include "texel_pass.h"
#include <math.h>

#define BLOOM_MAX_LEVELS 16

struct BloomAxis { int i[3]; }; // the source index of neighbour d = -1, 0, +1; outside [0, readDim) = no texel

// ComputeBloomDownscale.shader:76-88 / ComputeBloomUpscale.shader:48-57 for one axis of output pixel p
__device__ __forceinline__ BloomAxis bloom_src_index(int p, float readDim, float texel)
{
    const float base = (float)(8 * (p >> 3) - 1);
    const float uv = (base + 0.5f) * texel;
    BloomAxis a;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float off = (float)((p & 7) + d) * texel; // slot = (p & 7) + 1 + (d - 1)
        a.i[d] = (int)(readDim * (uv + off));           // |value| < 2^17: the conversion is the truncating one
    }
    return a;
}

__device__ __forceinline__ float4 bloom_tap(const float4* __restrict__ src, int W, int H, int x, int y)
{
    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    const float4 t = src[(size_t)y * (size_t)W + x];
    return make_float4(t.x, t.y, t.z, 1.0f); // load_lds
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

__device__ __forceinline__ float4 karis_avg(float4 c) // :38-47
{
    const float d = 1.0f + dot3f(c.x, c.y, c.z, 0.2126729f, 0.7151522f, 0.0721750f);
    return make_float4(c.x / d, c.y / d, c.z / d, c.w / d);
}

__global__ __launch_bounds__(256) void k_bloom_downscale(const float4* __restrict__ src, int RW, int RH, float4* __restrict__ dst, int W, int H,
                                                         float4 threshold, int useThreshold)
{
    const int x = texel_i(), y = texel_j();
    if (x >= W || y >= H) return;
    const BloomAxis ix = bloom_src_index(x, (float)RW, 1.0f / (float)W), iy = bloom_src_index(y, (float)RH, 1.0f / (float)H);
    const float4 A = bloom_tap(src, RW, RH, ix.i[0], iy.i[0]), B = bloom_tap(src, RW, RH, ix.i[1], iy.i[0]), C = bloom_tap(src, RW, RH, ix.i[2], iy.i[0]);
    const float4 F = bloom_tap(src, RW, RH, ix.i[0], iy.i[1]), G = bloom_tap(src, RW, RH, ix.i[1], iy.i[1]), Hh = bloom_tap(src, RW, RH, ix.i[2], iy.i[1]);
    const float4 K = bloom_tap(src, RW, RH, ix.i[0], iy.i[2]), L = bloom_tap(src, RW, RH, ix.i[1], iy.i[2]), M = bloom_tap(src, RW, RH, ix.i[2], iy.i[2]);

    const float4 sD = add4(add4(add4(A, B), G), F), sE = add4(add4(add4(B, C), Hh), G); // :108-111
    const float4 sI = add4(add4(add4(F, G), L), K), sJ = add4(add4(add4(G, Hh), M), L);
    const float4 D = mul4(sD, 0.25f), E = mul4(sE, 0.25f), I = mul4(sI, 0.25f), J = mul4(sJ, 0.25f);
    const float divX = 0.125f, divY = 0.03125f; // :113

    float4 c = karis_avg(mul4(add4(add4(add4(D, E), I), J), divX)); // :115-119
    c = add4(c, karis_avg(mul4(sD, divY)));
    c = add4(c, karis_avg(mul4(sE, divY)));
    c = add4(c, karis_avg(mul4(sI, divY)));
    c = add4(c, karis_avg(mul4(sJ, divY)));

    if (useThreshold) { // :21-35 quadratic_threshold(c, u_threshold.x, u_threshold.yzw)
        const float br = glsl_max(c.x, glsl_max(c.y, c.z));
        const float t = br - threshold.y;
        float rq = t < 0.0f ? 0.0f : (t > threshold.z ? threshold.z : t);
        rq = (threshold.w * rq) * rq;
        const float f = glsl_max(rq, br - threshold.x) / glsl_max(br, 1.0e-4f);
        c = mul4(c, f);
    }
    dst[(size_t)y * (size_t)W + x] = c;
}

template <bool DIRT>
__global__ __launch_bounds__(256) void k_bloom_upscale(const float4* __restrict__ src, int RW, int RH, float4* __restrict__ dst, int W, int H,
                                                       float bloomIntensity, float dirtIntensity, const float4* __restrict__ dirt, int DW, int DH)
{
    const int x = texel_i(), y = texel_j();
    if (x >= W || y >= H) return;
    const float texelX = 1.0f / (float)W, texelY = 1.0f / (float)H;
    const BloomAxis ix = bloom_src_index(x, (float)RW, texelX), iy = bloom_src_index(y, (float)RH, texelY);
    float4* __restrict__ o = dst + (size_t)y * (size_t)W + x;
    float4 out = *o; // :85

    float4 s = bloom_tap(src, RW, RH, ix.i[0], iy.i[0]); // :70-81
    s = add4(s, mul4(bloom_tap(src, RW, RH, ix.i[1], iy.i[0]), 2.0f));
    s = add4(s, bloom_tap(src, RW, RH, ix.i[2], iy.i[0]));
    s = add4(s, mul4(bloom_tap(src, RW, RH, ix.i[0], iy.i[1]), 2.0f));
    s = add4(s, mul4(bloom_tap(src, RW, RH, ix.i[1], iy.i[1]), 4.0f));
    s = add4(s, mul4(bloom_tap(src, RW, RH, ix.i[2], iy.i[1]), 2.0f));
    s = add4(s, bloom_tap(src, RW, RH, ix.i[0], iy.i[2]));
    s = add4(s, mul4(bloom_tap(src, RW, RH, ix.i[1], iy.i[2]), 2.0f));
    s = add4(s, bloom_tap(src, RW, RH, ix.i[2], iy.i[2]));
    const float4 bloom = mul4(s, 0.0625f); // :83

    out = add4(out, mul4(bloom, bloomIntensity)); // :86
    if (DIRT) { // :88-92
        const float u = ((float)x + 0.5f) * texelX, v = ((float)y + 0.5f) * texelY;
        const float4 t = mul4(sample_repeat_f4(dirt, DW, DH, u, v), dirtIntensity);
        out = add4(out, mul4(make_float4(t.x * bloom.x, t.y * bloom.y, t.z * bloom.z, t.w * bloom.w), bloomIntensity));
    }
    *o = out;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static int32_t bloom_half(int32_t d) { return (d >> 1) > 1 ? (d >> 1) : 1; }

// `big` and `small` are neighbouring levels of one chain
static bool bloom_pair_ok(SailorHipContext* ctx, const float* a, float* b, int32_t bigW, int32_t bigH, int32_t smallW, int32_t smallH)
{
    return ctx && aligned(a, 16) && aligned(b, 16) && a != b && extent_ok(bigW, bigH) && smallW == bloom_half(bigW) && smallH == bloom_half(bigH);
}
static bool bloom_dirt_ok(const float* dirt, int32_t w, int32_t h) { return !dirt || (aligned(dirt, 16) && extent_ok(w, h)); }

extern "C" {

size_t sailor_hip_mip_chain_texels(int32_t width, int32_t height, int32_t levels)
{
    if (!extent_ok(width, height) || levels < 0 || levels > BLOOM_MAX_LEVELS) return 0;
    size_t n = 0;
    for (int32_t l = 0; l < levels; l++) n += (size_t)((width >> l) > 1 ? (width >> l) : 1) * (size_t)((height >> l) > 1 ? (height >> l) : 1);
    return n;
}

int sailor_hip_bloom_downscale(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst, int32_t dstWidth, int32_t dstHeight,
                               const float* threshold4, int32_t useThreshold)
{
    if (!bloom_pair_ok(ctx, dSrc, dDst, srcWidth, srcHeight, dstWidth, dstHeight) || !threshold4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_bloom_downscale, texel_grid(dstWidth, dstHeight), dim3(256), (const float4*)dSrc, (int)srcWidth, (int)srcHeight, (float4*)dDst, (int)dstWidth,
                  (int)dstHeight, make_float4(threshold4[0], threshold4[1], threshold4[2], threshold4[3]), useThreshold ? 1 : 0);
    SAILOR_CHECK_LAUNCH(ctx, "k_bloom_downscale");
    return SAILOR_HIP_OK;
}

int sailor_hip_bloom_upscale(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst, int32_t dstWidth, int32_t dstHeight,
                             int32_t mipLevel, float bloomIntensity, float dirtIntensity, const float* dDirt, int32_t dirtWidth, int32_t dirtHeight)
{
    if (!bloom_pair_ok(ctx, dSrc, dDst, dstWidth, dstHeight, srcWidth, srcHeight) || !bloom_dirt_ok(dDirt, dirtWidth, dirtHeight) || dDirt == dDst)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (mipLevel == 1 && dDirt)
        sailor_launch(ctx, k_bloom_upscale<true>, texel_grid(dstWidth, dstHeight), dim3(256), (const float4*)dSrc, (int)srcWidth, (int)srcHeight, (float4*)dDst, (int)dstWidth,
                      (int)dstHeight, bloomIntensity, dirtIntensity, (const float4*)dDirt, (int)dirtWidth, (int)dirtHeight);
    else
        sailor_launch(ctx, k_bloom_upscale<false>, texel_grid(dstWidth, dstHeight), dim3(256), (const float4*)dSrc, (int)srcWidth, (int)srcHeight, (float4*)dDst, (int)dstWidth,
                      (int)dstHeight, bloomIntensity, dirtIntensity, (const float4*)nullptr, 0, 0);
    SAILOR_CHECK_LAUNCH(ctx, "k_bloom_upscale");
    return SAILOR_HIP_OK;
}

int sailor_hip_bloom(SailorHipContext* ctx, float* dChain, int32_t width, int32_t height, int32_t levels, const SailorBloomParams* params, const float* dDirt,
                     int32_t dirtWidth, int32_t dirtHeight)
{
    // every argument is checked before the first launch: a refused call records nothing
    if (!ctx || !aligned(dChain, 16) || !params || !extent_ok(width, height) || levels < 2 || levels > BLOOM_MAX_LEVELS || !bloom_dirt_ok(dDirt, dirtWidth, dirtHeight))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    float* level[BLOOM_MAX_LEVELS];
    int32_t w[BLOOM_MAX_LEVELS], h[BLOOM_MAX_LEVELS];
    for (int32_t l = 0; l < levels; l++) {
        level[l] = dChain + 4 * sailor_hip_mip_chain_texels(width, height, l);
        w[l] = l ? bloom_half(w[l - 1]) : width;
        h[l] = l ? bloom_half(h[l - 1]) : height;
    }
    float threshold[4];
    sailor_host_bloom_push_constants(params->threshold, params->knee, threshold); // BloomNode.cpp:89-93
    for (int32_t i = 0; i < levels - 1; i++) { // :99-116
        const int st = sailor_hip_bloom_downscale(ctx, level[i], w[i], h[i], level[i + 1], w[i + 1], h[i + 1], threshold, i == 0);
        if (st != SAILOR_HIP_OK) return st;
    }
    for (int32_t i = levels - 1; i >= 1; i--) { // :122-141
        const int st = sailor_hip_bloom_upscale(ctx, level[i], w[i], h[i], level[i - 1], w[i - 1], h[i - 1], i, params->bloomIntensity, params->dirtIntensity, dDirt,
                                                dirtWidth, dirtHeight);
        if (st != SAILOR_HIP_OK) return st;
    }
    return SAILOR_HIP_OK;
}

} // extern "C"
