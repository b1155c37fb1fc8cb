// The post effects the shipped frame graph names but does not run (tests/golden/DefaultRenderer.renderer:157-181, :355-366, and the blur chain its unused
// QuarterMain1 / QuarterMain2 targets are there for), for gfx950.
//
// Replaces the GPU work of
//   * PostProcess with Content/Shaders/Blur.shader:66-98 without RADIAL and EVSM -> GaussianBlur (Lighting.glsl:129-159)  -> k_blur_gauss
//   * the same shader under RADIAL (:78-89; it wins over EVSM by the #ifdef order)                                          -> k_blur_radial
//   * PostProcess with Content/Shaders/ChromaticAberation.shader:62-73                                                      -> k_chromatic_aberration
//   * Blit of a whole scaled image with VK_FILTER_LINEAR (FrameGraph/BlitNode.cpp:88-96)                                    -> k_blit_linear<CHANNELS>
// Images are fp32 RGBA float4 planes, 16-byte aligned (the blit also takes one-channel planes); row 0 = top; texel (i, j) of a w x h target has
// fragTexcoord = ((i + 0.5) / w, (j + 0.5) / h); source and target extents are independent.
//
// Arithmetic is evaluated exactly as the shaders write it, left to right, one IEEE rounding per operation (-ffp-contract=off, IEEE division, denormals
// kept).  tests/effects_ref.py restates it in NumPy float32 and the kernels reproduce it bit for bit.
//
// Decisions where "as written" needs one (Blur.shader line numbers):
//   * texelSize = 1.0f / textureSize(colorSampler, 0) (:68) is uniform per draw: the entry point computes (1.0f / srcW, 1.0f / srcH) once on the host.
//     VERTICAL zeroes x (:70-72), HORIZONTAL zeroes y (:74-76).  Neither define gives the diagonal, both put every tap at uv: all four are legal, as written.
//   * Gauss: radius = uint(data.blurRadius.x) truncates (:94); blurRadius = min(radius, 12) (Lighting.glsl:147); the row weights[blurRadius - 1] is passed by
//     value, as shadow_blur.hip passes its rows.  The loop (:151-156) runs i = 0 .. blurRadius - 1: off = float(i) * texelSize,
//     color = texture(uv + off) + texture(uv - off), pixelSum = pixelSum + color * w[i].  Tap 0 reads the centre twice: kept.  blurRadius == 0 writes rgb 0.
//   * The shader assigns only outColor.xyz (:94): alpha is undefined in the reference.  THIS PATH WRITES ALPHA 0.0f.
//   * RADIAL: direction = ((blurCenter.xy - uv) * texelSize) * blurRadius.x (:79), texelSize zeroed by HORIZONTAL / VERTICAL as above; the loop is
//     for (index = 0; float(index) < blurSampleCount.x; ++index) { sum += texture(uv); uv += direction; } (:83-87) and the result sum / blurSampleCount.x
//     (:89), one division per component, all four channels.  A fractional count runs ceil(count) taps and divides by the fraction.  The count is capped at
//     256 by the entry point -- the reference has no cap; this one is this path's, like the motion blur's 64.
//   * Every texture() of the three PostProcess kernels: bilinear, clamp-to-edge, the taps and weights of sampling.h evaluated per fetch with the saturating
//     float -> int conversion (sample_clamp_f4_saturating): the coordinates are driven by parameters (a radius of 1e30, an offset of 1e38) and may leave
//     the int range or turn into inf - inf.
// ChromaticAberation.shader line numbers:
//   * x = abs(u - 0.5f) / 0.5f, d = pow(x, 4) = (x * x) * (x * x) (:66): a pow with a small integer exponent is written as products, the convention of
//     sky.hip / sky_stars.hip.  Per channel c: p = offset.c * d, ONE fetch at (u - p, v - p) (:68-70); out = (r of the first fetch, g of the second, b of the
//     third, 1) (:72).  The first fetch (:64) is overwritten at :72 and is not made.
// The Linear blit: destination texel (i, j) is texture() of the source at the texel's own fragTexcoord, the same clamp-to-edge bilinear taps with the plain
// conversion (bilinear_taps): the coordinates lie in (0, 1) whatever the arguments.  A 2 : 1 blit of power-of-two extents puts every coordinate midway
// between two texel centres on both axes: the 2 x 2 mean with weights of exactly 0.5, in lerp2's order.
//
// Shape.  One texel per lane, 256-thread blocks of 64 x 4 texels (texel_pass.h), no LDS, no barrier, no atomics, colour moved as 16-byte loads and stores;
// the parameters are kernel arguments (scalar registers).  All four are memory-bound gathers whose taps neighbouring lanes share: the Gauss pass reads
// 2 x 4 texels per step from rows (HORIZONTAL) or columns (VERTICAL) the wave's other lanes read too, so the vector L1 / L2 absorb the reuse.
#include "common.h"
#include "sampling.h"
#include "texel_pass.h"
#include <math.h>

#define GAUSS_STEP_COUNT 12
struct GaussRow { float w[GAUSS_STEP_COUNT]; }; // weights[blurRadius - 1] of Lighting.glsl:133-145

// Lighting.glsl:133-145 (the table GaussianBlur_Evsm repeats at :87-99)
static const float kGaussWeights[GAUSS_STEP_COUNT][GAUSS_STEP_COUNT] = {
    { 0.5f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 },
    { 0.281088f, 0.218912f, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 },
    { 0.197159f, 0.176426f, 0.126415f, 0, 0, 0, 0, 0, 0, 0, 0, 0 },
    { 0.152068f, 0.142855f, 0.118431f, 0.0866459f, 0, 0, 0, 0, 0, 0, 0, 0 },
    { 0.123827f, 0.118971f, 0.105518f, 0.0863909f, 0.0652929f, 0, 0, 0, 0, 0, 0, 0 },
    { 0.104454f, 0.101593f, 0.0934699f, 0.0813492f, 0.0669741f, 0.0521595f, 0, 0, 0, 0, 0, 0 },
    { 0.0903332f, 0.0885083f, 0.083252f, 0.0751759f, 0.0651684f, 0.0542336f, 0.0433285f, 0, 0, 0, 0, 0 },
    { 0.07958f, 0.0783462f, 0.0747585f, 0.0691403f, 0.061977f, 0.0538465f, 0.0453433f, 0.0370081f, 0, 0, 0, 0 },
    { 0.0711171f, 0.0702445f, 0.0676904f, 0.0636383f, 0.0583697f, 0.0522315f, 0.0455989f, 0.0388376f, 0.0322721f, 0, 0, 0 },
    { 0.0642825f, 0.0636429f, 0.0617619f, 0.0587498f, 0.0547779f, 0.0500633f, 0.0448484f, 0.0393811f, 0.0338957f, 0.0285966f, 0, 0 },
    { 0.0586472f, 0.0581645f, 0.0567402f, 0.0544433f, 0.0513831f, 0.0476999f, 0.0435548f, 0.039118f, 0.0345572f, 0.0300277f, 0.0256641f, 0 },
    { 0.0539209f, 0.0535478f, 0.0524437f, 0.050654f, 0.0482506f, 0.0453272f, 0.0419936f, 0.0383686f, 0.034573f, 0.0307232f, 0.0269255f, 0.0232718f } };

// ---- a. Blur.shader without RADIAL and EVSM ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blur_gauss(const float4* __restrict__ src, int SW, int SH, float4* __restrict__ dst, int W, int H, float texelX,
                                                    float texelY, int blurRadius, const GaussRow K)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    float r = 0.0f, g = 0.0f, b = 0.0f; // Lighting.glsl:149
#pragma unroll
    for (int k = 0; k < GAUSS_STEP_COUNT; k++) { // :151-156; unrolled so that K.w[k] names a register
        if (k >= blurRadius) break;
        const float offX = (float)k * texelX, offY = (float)k * texelY;
        const float4 p = sample_clamp_f4_saturating(src, SW, SH, u + offX, v + offY);
        const float4 m = sample_clamp_f4_saturating(src, SW, SH, u - offX, v - offY);
        r = r + (p.x + m.x) * K.w[k]; g = g + (p.y + m.y) * K.w[k]; b = b + (p.z + m.z) * K.w[k];
    }
    dst[(size_t)j * (size_t)W + i] = make_float4(r, g, b, 0.0f); // outColor.xyz only (Blur.shader:94): alpha is this path's 0
}

// ---- b. Blur.shader under RADIAL ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blur_radial(const float4* __restrict__ src, int SW, int SH, float4* __restrict__ dst, int W, int H, float texelX,
                                                     float texelY, float radius, float centerX, float centerY, float sampleCount)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const float dirX = ((centerX - u) * texelX) * radius, dirY = ((centerY - v) * texelY) * radius; // Blur.shader:79
    float r = 0.0f, g = 0.0f, b = 0.0f, a = 0.0f;
    for (int index = 0; (float)index < sampleCount; ++index) { // :83-87; the entry point keeps the count within [1, 256]
        const float4 c = sample_clamp_f4_saturating(src, SW, SH, u, v);
        r = r + c.x; g = g + c.y; b = b + c.z; a = a + c.w;
        u = u + dirX; v = v + dirY;
    }
    dst[(size_t)j * (size_t)W + i] = make_float4(r / sampleCount, g / sampleCount, b / sampleCount, a / sampleCount); // :89
}

// ---- c. ChromaticAberation.shader ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_chromatic_aberration(const float4* __restrict__ src, int SW, int SH, float4* __restrict__ dst, int W, int H,
                                                              float offsetR, float offsetG, float offsetB)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const float x = fabsf(u - 0.5f) / 0.5f;
    const float d = (x * x) * (x * x); // :66
    const float pr = offsetR * d, pg = offsetG * d, pb = offsetB * d;
    const float4 rValue = sample_clamp_f4_saturating(src, SW, SH, u - pr, v - pr); // :68
    const float4 gValue = sample_clamp_f4_saturating(src, SW, SH, u - pg, v - pg); // :69
    const float4 bValue = sample_clamp_f4_saturating(src, SW, SH, u - pb, v - pb); // :70
    dst[(size_t)j * (size_t)W + i] = make_float4(rValue.x, gValue.y, bValue.z, 1.0f); // :72
}

// ---- d. the scaled blit with VK_FILTER_LINEAR ----------------------------------------------------------------------------------------------------
template <int CHANNELS>
__global__ __launch_bounds__(256) void k_blit_linear(const float* __restrict__ src, int SW, int SH, float* __restrict__ dst, int W, int H)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const size_t at = (size_t)j * (size_t)W + i;
    if (CHANNELS == 4) {
        reinterpret_cast<float4*>(dst)[at] = sample_clamp_f4(reinterpret_cast<const float4*>(src), SW, SH, u, v);
    } else {
        const BilinearTaps t = bilinear_taps(SW, SH, u, v);
        const float* __restrict__ r0 = src + (size_t)t.y0 * (size_t)SW;
        const float* __restrict__ r1 = src + (size_t)t.y1 * (size_t)SW;
        dst[at] = lerp2(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.ax, t.ay);
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------------------------
#define RADIAL_MAX_SAMPLES 256.0f

// what the three PostProcess entry points refuse alike: a null or misaligned plane, an extent outside extent_ok, an output that overlaps its source (taps
// read what other lanes write)
static bool planes_ok(const float* dSrc, int32_t srcWidth, int32_t srcHeight, const float* dOut, int32_t width, int32_t height, size_t texelBytes)
{
    return aligned(dSrc, texelBytes) && aligned(dOut, texelBytes) && extent_ok(srcWidth, srcHeight) && extent_ok(width, height) &&
           !overlaps(dOut, (size_t)width * height * texelBytes, dSrc, (size_t)srcWidth * srcHeight * texelBytes);
}

extern "C" {

int sailor_hip_blur(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, const SailorBlurParams* params, uint32_t flags, float* dOut,
                    int32_t width, int32_t height)
{
    if (!ctx || !params || !planes_ok(dSrc, srcWidth, srcHeight, dOut, width, height, 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (flags & ~(SAILOR_BLUR_HORIZONTAL | SAILOR_BLUR_VERTICAL | SAILOR_BLUR_RADIAL)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const float radius = params->blurRadius[0];
    const float texelX = (flags & SAILOR_BLUR_VERTICAL) ? 0.0f : 1.0f / (float)srcWidth;    // Blur.shader:68-72
    const float texelY = (flags & SAILOR_BLUR_HORIZONTAL) ? 0.0f : 1.0f / (float)srcHeight; // :74-76
    const dim3 grid = texel_grid(width, height), block(256);
    if (flags & SAILOR_BLUR_RADIAL) {
        const float count = params->blurSampleCount[0];
        // the loop runs while float(index) < count: a NaN, an infinity or anything outside [1, 256] is refused rather than run without an end
        if (!isfinite(radius) || !isfinite(params->blurCenter[0]) || !isfinite(params->blurCenter[1]) || !(count >= 1.0f && count <= RADIAL_MAX_SAMPLES))
            return SAILOR_HIP_ERR_INVALID_ARGUMENT;
        SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
        sailor_launch(ctx, k_blur_radial, grid, block, (const float4*)dSrc, (int)srcWidth, (int)srcHeight, (float4*)dOut, (int)width, (int)height, texelX, texelY,
                      radius, params->blurCenter[0], params->blurCenter[1], count);
        SAILOR_CHECK_LAUNCH(ctx, "k_blur_radial");
        return SAILOR_HIP_OK;
    }
    if (!(radius >= 0.0f && radius < 4294967296.0f)) return SAILOR_HIP_ERR_INVALID_ARGUMENT; // uint() of a NaN, a negative or >= 2^32 is undefined
    const uint32_t truncated = (uint32_t)radius;                                              // :94
    const int blurRadius = truncated < GAUSS_STEP_COUNT ? (int)truncated : GAUSS_STEP_COUNT;  // Lighting.glsl:147
    GaussRow K;
    memset(&K, 0, sizeof K);
    if (blurRadius > 0) memcpy(K.w, kGaussWeights[blurRadius - 1], sizeof K.w);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_blur_gauss, grid, block, (const float4*)dSrc, (int)srcWidth, (int)srcHeight, (float4*)dOut, (int)width, (int)height, texelX, texelY,
                  blurRadius, K);
    SAILOR_CHECK_LAUNCH(ctx, "k_blur_gauss");
    return SAILOR_HIP_OK;
}

int sailor_hip_chromatic_aberration(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, const SailorChromaticAberrationParams* params,
                                    float* dOut, int32_t width, int32_t height)
{
    if (!ctx || !params || !planes_ok(dSrc, srcWidth, srcHeight, dOut, width, height, 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!isfinite(params->offset[0]) || !isfinite(params->offset[1]) || !isfinite(params->offset[2])) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_chromatic_aberration, texel_grid(width, height), dim3(256), (const float4*)dSrc, (int)srcWidth, (int)srcHeight, (float4*)dOut, (int)width,
                  (int)height, params->offset[0], params->offset[1], params->offset[2]);
    SAILOR_CHECK_LAUNCH(ctx, "k_chromatic_aberration");
    return SAILOR_HIP_OK;
}

int sailor_hip_blit_linear(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst, int32_t dstWidth, int32_t dstHeight,
                           int32_t channels)
{
    if (!ctx || (channels != 1 && channels != 4) || !planes_ok(dSrc, srcWidth, srcHeight, dDst, dstWidth, dstHeight, (size_t)channels * 4))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid = texel_grid(dstWidth, dstHeight), block(256);
    if (channels == 4) sailor_launch(ctx, k_blit_linear<4>, grid, block, dSrc, (int)srcWidth, (int)srcHeight, dDst, (int)dstWidth, (int)dstHeight);
    else sailor_launch(ctx, k_blit_linear<1>, grid, block, dSrc, (int)srcWidth, (int)srcHeight, dDst, (int)dstWidth, (int)dstHeight);
    SAILOR_CHECK_LAUNCH(ctx, "k_blit_linear");
    return SAILOR_HIP_OK;
}

} // extern "C"
