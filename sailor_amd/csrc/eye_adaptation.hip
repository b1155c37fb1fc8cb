// Eye adaptation and tone mapping for gfx950: the EyeAdaptation node, the first node behind the two RenderScene passes
// (tests/golden/DefaultRenderer.renderer:307-319).
//
// Replaces the three GPU steps recorded by EyeAdaptationNode::Process (FrameGraph/EyeAdaptationNode.cpp:22-221):
//   * the Dispatch of Content/Shaders/ComputeHistogram.shader (:173-176): a 256-bin log-luminance histogram of the HDR target,
//   * the Dispatch of Content/Shaders/ComputeAverageLuminance.shader (:179-182): one block that reduces the histogram to a
//     temporally smoothed average luminance and zeroes the counts for the next frame,
//   * the full-screen draw of Content/Shaders/Tonemapping.shader (:192-218) with Content/Shaders/Formats.glsl:1-51.
// Targets are kept in their fp32 canonical form (FrameGraphParser.cpp:196): float4 radiance in, float4 out, one fp32 word of adapted
// luminance; nothing is rounded to half.
//
// Shapes.
//   k_luminance_histogram  The reference launches one 16 x 16 block per 256 pixels (32 400 at 4K), each ending in 256 global atomics on the
//       same 256 words.  Here: a persistent grid (2 blocks of 16 waves per CU); a wave takes 256 consecutive pixels of a row at a time as four
//       independent 1 KiB float4 loads, issued one step ahead of the step whose bins are being computed; every wave owns a private LDS histogram, replicated over 4 lane groups (lane & 3), and adds to it
//       with non-returning ds_add_u32.  A tone-mapped frame piles its pixels into a few bins, so the lanes that share the FIRST lane's bin
//       are combined by ballot + popcount into one add (a one-bin image costs one LDS atomic per 64 pixels); what is left spreads over the
//       replicas.  One flush per block: thread b sums bin b over waves and replicas and issues one non-returning global atomic if non-zero
//       (at most 512 x 256 per launch against the reference's 8.3 M).  Counts are integers: any order is exact.
//       LDS: 16 waves x 256 bins x 4 replicas x 4 B = 64 KiB per block, so 160 KiB hold the 2 blocks = 32 waves a CU can run at all (<= 64 VGPRs).
//   k_average_luminance    One 256-thread block, as the reference has it.  log2 / exp2 are the fixed fp32 algorithms of canonical_math.h, not v_log_f32 /
//       v_exp_f32: tests/eye_adaptation_ref.py restates them and reproduces bins and luminance bit for bit.
//   k_tonemap<OPS>         A float4-in, float4-out streaming kernel, four pixels in flight per lane; the operator set is a template
//       parameter (six distinct bodies), the average luminance is one uniform load, 1 / partial(whitePoint) comes in as an argument.
//
// Arithmetic is evaluated exactly as written, one IEEE rounding per operation (-ffp-contract=off, IEEE division); GLSL fixes no order, this
// file does: dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; mat3 * v row by row with that dot (the GLSL constructors are column-major);
// vec3 / float = three divisions; every literal is its fp32 value.
//
// Kept quirks: the histogram's dispatch is extent / 16 by integer division (EyeAdaptationNode.cpp:173-174), so the right / bottom
// remainder of a size that is no multiple of 16 is not counted while numPixels stays width x height; the weighted sum is uint32 and wraps
// at 8K; a black pixel under LUMINANCE divides by X + Y + Z = 0 and comes out NaN (Formats.glsl:18).
// Defined where GLSL leaves it open: a NaN luminance counts in bin 0, +inf in bin 255, no input indexes outside the 256 bins; clamp()
// is glsl_saturate of common.h, which passes a NaN through.
#include "common.h"
#include "canonical_math.h"
#include <math.h>

#define EA_BINS 256
#define EA_REPLICAS 4
#define EA_HIST_WAVES 16
#define EA_BLOCKS_PER_CU 2
#define EA_STATE_WORDS 272 // 256 counts, the adapted luminance at word 256, padding to whole 64-byte lines

// ---- histogram ------------------------------------------------------------------------------------------------------------------------
// ComputeHistogram.shader:37-54 colorToBin
__device__ __forceinline__ uint32_t color_to_bin(const float4 c, const float minLog, const float invRange)
{
    const float lum = (c.x * 0.2125f + c.y * 0.7154f) + c.z * 0.0721f; // :40
    if (!(lum >= 0.005f)) return 0u;                                    // :43-46 (and NaN, which GLSL leaves open)
    if (lum == INFINITY) return 255u;
    float t = (canonical_log2f(lum) - minLog) * invRange;               // :50
    t = glsl_saturate(t);
    const float f = t * 254.0f + 1.0f;                                  // :53
    return f < 256.0f ? (uint32_t)f : 255u;                             // (only NaN constants get past the clamp)
}

__global__ __launch_bounds__(64 * EA_HIST_WAVES) void k_luminance_histogram(const float4* __restrict__ color, int W, int rowCount, int countW,
                                                                            float minLog, float invRange, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t hist[EA_HIST_WAVES][EA_BINS * EA_REPLICAS];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < EA_HIST_WAVES * EA_BINS * EA_REPLICAS; i += 64 * EA_HIST_WAVES) (&hist[0][0])[i] = 0u;
    __syncthreads();
    uint32_t* h = hist[wave];
    const uint32_t replica = (uint32_t)lane & (EA_REPLICAS - 1);
    const int chunks = (countW + 255) >> 8; // 256 pixels of one row per wave and step
    const int tasks = rowCount * chunks;
    const int stride = (int)gridDim.x * EA_HIST_WAVES;
    int t = (int)blockIdx.x * EA_HIST_WAVES + wave;
    float4 p[4], q[4];
    // one step ahead: the loads of the next 256 pixels are in flight while this step's bins are computed and added
    auto fetch = [&](int task, float4 (&dst)[4]) {
        const int row = task / chunks, x0 = (task - row * chunks) * 256 + lane;
        const float4* __restrict__ src = color + (size_t)row * (size_t)W;
#pragma unroll
        for (int k = 0; k < 4; k++) dst[k] = x0 + 64 * k < countW ? src[x0 + 64 * k] : make_float4(0, 0, 0, 0);
    };
    if (t < tasks) fetch(t, p);
    for (; t < tasks; t += stride) {
        const int x0 = (t % chunks) * 256 + lane;
        if (t + stride < tasks) fetch(t + stride, q);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool counted = x0 + 64 * k < countW;
            const uint32_t bin = counted ? color_to_bin(p[k], minLog, invRange) : 0xffffffffu;
            // the lanes that share the first lane's bin become one add
            const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
            const bool same = bin == first;
            const unsigned long long mask = __ballot(same);
            if (lane == 0 && first != 0xffffffffu) __hip_atomic_fetch_add(&h[first * EA_REPLICAS], (uint32_t)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (!same && counted) __hip_atomic_fetch_add(&h[bin * EA_REPLICAS + replica], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = q[k];
    }
    __syncthreads();
    if (tid < EA_BINS) { // ComputeHistogram.shader:82, once per block instead of once per 256 pixels
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < EA_HIST_WAVES; w++) {
            const uint4 v = *reinterpret_cast<const uint4*>(&hist[w][tid * EA_REPLICAS]);
            s += (v.x + v.y) + (v.z + v.w);
        }
        if (s) __hip_atomic_fetch_add(&counts[tid], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- average --------------------------------------------------------------------------------------------------------------------------
// ComputeAverageLuminance.shader:39-78
__global__ __launch_bounds__(EA_BINS) void k_average_luminance(uint32_t* __restrict__ counts, float* __restrict__ luminance, float minLog, float logRange,
                                                               float numPixels, float timeCoeff)
{
    __shared__ uint32_t shared[EA_BINS];
    const uint32_t i = threadIdx.x;
    const uint32_t countForThisBin = counts[i]; // :42
    shared[i] = countForThisBin * i;            // :43 (uint32: wraps)
    __syncthreads();
    counts[i] = 0u;                             // :48
    for (uint32_t cutoff = EA_BINS >> 1; cutoff > 0; cutoff >>= 1) { // :51-59
        if (i < cutoff) shared[i] += shared[i + cutoff];
        __syncthreads();
    }
    if (i == 0) {
        const float lit = numPixels - (float)countForThisBin;
        const float weightedLogAverage = (float)shared[0] / (lit > 1.0f ? lit : 1.0f) - 1.0f;      // :67
        const float weightedAvgLum = canonical_exp2f(((weightedLogAverage / 254.0f) * logRange) + minLog); // :70
        const float last = *luminance;                                                            // :74
        *luminance = last + (weightedAvgLum - last) * timeCoeff;                                    // :75-76
    }
}

__global__ void k_eye_adaptation_reset(uint32_t* __restrict__ state, float initialLuminance)
{
    const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
    if (i < EA_STATE_WORDS) state[i] = i == EA_BINS ? __float_as_uint(initialLuminance) : 0u;
}

// ---- tone map -------------------------------------------------------------------------------------------------------------------------
struct TonemapArgs {
    float whiteScale[3]; // 1 / uncharted2_tonemap_partial(whitePoint), Tonemapping.shader:129
    float exposure;
};

__host__ __device__ __forceinline__ float uncharted2_partial(float x) // Tonemapping.shader:115-124
{
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}
__device__ __forceinline__ float aces_fit(float v) // :89-94
{
    const float a = v * (v + 0.0245786f) - 0.000090537f;
    const float b = v * (0.983729f * v + 0.4329510f) + 0.238081f;
    return a / b;
}

#define EA_OP_ACES 1
#define EA_OP_UNCHARTED2 2
#define EA_OP_LUMINANCE 4

template <int OPS>
__device__ __forceinline__ float4 tonemap_pixel(const float4 in, const float scale, const TonemapArgs& A)
{
    constexpr bool ACES = (OPS & EA_OP_ACES) != 0, U2 = !ACES && (OPS & EA_OP_UNCHARTED2) != 0, LUM = (OPS & EA_OP_LUMINANCE) != 0; // :150-154: ACES wins
    float cx, cy, cz, Yx = 0.0f, Yy = 0.0f;
    if (LUM) { // :142-148 + Formats.glsl:1-25
        const float X = dot3f(0.4124564f, 0.3575761f, 0.1804375f, in.x, in.y, in.z);
        const float Y = dot3f(0.2126729f, 0.7151522f, 0.0721750f, in.x, in.y, in.z);
        const float Z = dot3f(0.0193339f, 0.1191920f, 0.9503041f, in.x, in.y, in.z);
        const float inv = 1.0f / dot3f(X, Y, Z, 1.0f, 1.0f, 1.0f);
        Yx = X * inv; Yy = Y * inv;
        cx = cy = cz = Y / scale;
    } else { cx = in.x / scale; cy = in.y / scale; cz = in.z / scale; } // :140
    if (ACES) { // :96-109
        const float ix = aces_fit(dot3f(0.59719f, 0.35458f, 0.04823f, cx, cy, cz));
        const float iy = aces_fit(dot3f(0.07600f, 0.90834f, 0.01566f, cx, cy, cz));
        const float iz = aces_fit(dot3f(0.02840f, 0.13383f, 0.83777f, cx, cy, cz));
        cx = glsl_saturate(dot3f(1.60475f, -0.53108f, -0.07367f, ix, iy, iz));
        if (!LUM) { // under LUMINANCE only color.x reaches the output (:157)
            cy = glsl_saturate(dot3f(-0.10208f, 1.10813f, -0.00605f, ix, iy, iz));
            cz = glsl_saturate(dot3f(-0.00327f, -0.07276f, 1.07602f, ix, iy, iz));
        }
    } else if (U2) { // :126-131
        cx = uncharted2_partial(cx * A.exposure) * A.whiteScale[0];
        if (!LUM) {
            cy = uncharted2_partial(cy * A.exposure) * A.whiteScale[1];
            cz = uncharted2_partial(cz * A.exposure) * A.whiteScale[2];
        }
    }
    if (LUM) { // :157 + Formats.glsl:27-51
        const float X = cx * Yx / Yy, Y = cx, Z = cx * ((1.0f - Yx) - Yy) / Yy;
        cx = dot3f(3.2404542f, -1.5371385f, -0.4985314f, X, Y, Z);
        cy = dot3f(-0.9692660f, 1.8760108f, 0.0415560f, X, Y, Z);
        cz = dot3f(0.0556434f, -0.2040259f, 1.0572252f, X, Y, Z);
    }
    return make_float4(cx, cy, cz, in.w); // alpha is the sampled texel's (:137)
}

template <int OPS>
__global__ __launch_bounds__(256) void k_tonemap(const float4* __restrict__ src, float4* __restrict__ dst, size_t count, const float* __restrict__ luminance,
                                                 const TonemapArgs A)
{
    const float scale = 9.6f * *luminance + 0.0001f; // :138-140; a uniform (scalar) load
    const size_t stride = (size_t)gridDim.x * 1024;
    for (size_t base = (size_t)blockIdx.x * 1024 + threadIdx.x; base < count; base += stride) {
        float4 p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = base + 256 * k < count ? src[base + 256 * k] : make_float4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (base + 256 * k < count) dst[base + 256 * k] = tonemap_pixel<OPS>(p[k], scale, A);
    }
}

template <int OPS>
static void launch_tonemap(SailorHipContext* ctx, const float4* src, float4* dst, size_t count, const float* lum, const TonemapArgs& A)
{
    size_t blocks = (count + 1023) / 1024;
    const size_t cap = (size_t)ctx->numCUs * 8; // 8 blocks = 32 waves per CU, grid-stride beyond
    if (blocks > cap) blocks = cap;
    sailor_launch(ctx, k_tonemap<OPS>, dim3((unsigned)blocks), dim3(256), src, dst, count, lum, A);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------
static bool ea_state_ok(const void* dState) { return dState && ((uintptr_t)dState & 15) == 0; }

extern "C" {

size_t sailor_hip_eye_adaptation_state_size(void) { return EA_STATE_WORDS * sizeof(uint32_t); }

int sailor_hip_eye_adaptation_state_views(const void* dState, const uint32_t** outCounts, const float** outLuminance)
{
    if (!ea_state_ok(dState)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (outCounts) *outCounts = (const uint32_t*)dState;
    if (outLuminance) *outLuminance = (const float*)((const uint32_t*)dState + EA_BINS);
    return SAILOR_HIP_OK;
}

int sailor_hip_eye_adaptation_reset(SailorHipContext* ctx, void* dState, float initialLuminance)
{
    if (!ctx || !ea_state_ok(dState)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_eye_adaptation_reset, dim3((EA_STATE_WORDS + 255) / 256), dim3(256), (uint32_t*)dState, initialLuminance);
    SAILOR_CHECK_LAUNCH(ctx, "k_eye_adaptation_reset");
    return SAILOR_HIP_OK;
}

int sailor_hip_luminance_histogram(SailorHipContext* ctx, const float* dColor, int32_t width, int32_t height, const SailorBand* band,
                                   const SailorEyeAdaptationConstants* constants, void* dState)
{
    if (!ctx || !band || !constants || !ea_state_ok(dState) || width <= 0 || height <= 0) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!sailor_hip_band_is_valid(width, height, band)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (band->fbRowCount == 0) return SAILOR_HIP_OK; // a rank without rows (more ranks than tile rows) holds no buffer
    if (!dColor || ((uintptr_t)dColor & 15)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    // EyeAdaptationNode.cpp:173-174: extent / 16 groups of 16 x 16, from the image's first row and column
    const int countW = width / 16 * 16, countH = height / 16 * 16;
    const int rowEnd = band->fbRowBegin + band->fbRowCount < countH ? band->fbRowBegin + band->fbRowCount : countH;
    const int rowCount = rowEnd - band->fbRowBegin;
    if (countW <= 0 || rowCount <= 0) return SAILOR_HIP_OK;
    const long long tasks = (long long)rowCount * ((countW + 255) / 256);
    if (tasks >= (1ll << 30)) return SAILOR_HIP_ERR_UNSUPPORTED; // 32-bit task indices
    long long blocks = (tasks + EA_HIST_WAVES - 1) / EA_HIST_WAVES;
    if (blocks > (long long)ctx->numCUs * EA_BLOCKS_PER_CU) blocks = (long long)ctx->numCUs * EA_BLOCKS_PER_CU;
    sailor_launch(ctx, k_luminance_histogram, dim3((unsigned)blocks), dim3(64 * EA_HIST_WAVES), (const float4*)dColor, (int)width, rowCount, countW,
                  constants->minLog2Luminance, constants->invLog2LuminanceRange, (uint32_t*)dState);
    SAILOR_CHECK_LAUNCH(ctx, "k_luminance_histogram");
    return SAILOR_HIP_OK;
}

int sailor_hip_average_luminance(SailorHipContext* ctx, const SailorEyeAdaptationConstants* constants, void* dState)
{
    if (!ctx || !constants || !ea_state_ok(dState)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_average_luminance, dim3(1), dim3(EA_BINS), (uint32_t*)dState, (float*)((uint32_t*)dState + EA_BINS), constants->minLog2Luminance,
                  constants->log2LuminanceRange, constants->numPixels, constants->timeCoeff);
    SAILOR_CHECK_LAUNCH(ctx, "k_average_luminance");
    return SAILOR_HIP_OK;
}

int sailor_hip_tonemap(SailorHipContext* ctx, const float* dColor, float* dOut, int32_t width, int32_t height, const SailorBand* band,
                       uint32_t operatorFlags, const float* whitePoint4, float exposure, const void* dState)
{
    if (!ctx || !band || !whitePoint4 || !ea_state_ok(dState) || width <= 0 || height <= 0) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!sailor_hip_band_is_valid(width, height, band)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (operatorFlags & ~(uint32_t)(SAILOR_TONEMAP_ACES | SAILOR_TONEMAP_UNCHARTED2 | SAILOR_TONEMAP_LUMINANCE)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const size_t count = (size_t)band->fbRowCount * (size_t)width;
    if (!count) return SAILOR_HIP_OK; // a rank without rows holds no buffers
    if (!dColor || !dOut || dColor == dOut || (((uintptr_t)dColor | (uintptr_t)dOut) & 15)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    TonemapArgs A;
    for (int c = 0; c < 3; c++) A.whiteScale[c] = 1.0f / uncharted2_partial(whitePoint4[c]); // Tonemapping.shader:129, once per draw
    A.exposure = exposure;
    const float4* src = (const float4*)dColor;
    float4* dst = (float4*)dOut;
    const float* lum = (const float*)((const uint32_t*)dState + EA_BINS);
    uint32_t ops = operatorFlags;
    if (ops & SAILOR_TONEMAP_ACES) ops &= ~(uint32_t)SAILOR_TONEMAP_UNCHARTED2; // #if ACES #elif UNCHARTED2 (:150-154)
    switch (ops) {
    case 0: launch_tonemap<0>(ctx, src, dst, count, lum, A); break;
    case EA_OP_ACES: launch_tonemap<EA_OP_ACES>(ctx, src, dst, count, lum, A); break;
    case EA_OP_UNCHARTED2: launch_tonemap<EA_OP_UNCHARTED2>(ctx, src, dst, count, lum, A); break;
    case EA_OP_LUMINANCE: launch_tonemap<EA_OP_LUMINANCE>(ctx, src, dst, count, lum, A); break;
    case EA_OP_ACES | EA_OP_LUMINANCE: launch_tonemap<EA_OP_ACES | EA_OP_LUMINANCE>(ctx, src, dst, count, lum, A); break;
    default: launch_tonemap<EA_OP_UNCHARTED2 | EA_OP_LUMINANCE>(ctx, src, dst, count, lum, A); break;
    }
    SAILOR_CHECK_LAUNCH(ctx, "k_tonemap");
    return SAILOR_HIP_OK;
}

int sailor_hip_eye_adaptation(SailorHipContext* ctx, const float* dColor, float* dOut, int32_t width, int32_t height,
                              const SailorEyeAdaptationConstants* constants, uint32_t operatorFlags, const float* whitePoint4, float exposure, void* dState)
{
    // every argument is checked before the first launch: a refused call records nothing
    if (!ctx || !dColor || !dOut || !constants || !whitePoint4 || !ea_state_ok(dState) || width <= 0 || height <= 0) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (dColor == dOut || (((uintptr_t)dColor | (uintptr_t)dOut) & 15)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (operatorFlags & ~(uint32_t)(SAILOR_TONEMAP_ACES | SAILOR_TONEMAP_UNCHARTED2 | SAILOR_TONEMAP_LUMINANCE)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SailorBand whole;
    if (sailor_hip_band_whole_frame(width, height, &whole) != SAILOR_HIP_OK) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    int st = sailor_hip_luminance_histogram(ctx, dColor, width, height, &whole, constants, dState); // EyeAdaptationNode.cpp:173-176
    if (st != SAILOR_HIP_OK) return st;
    st = sailor_hip_average_luminance(ctx, constants, dState);                                       // :179-182
    if (st != SAILOR_HIP_OK) return st;
    return sailor_hip_tonemap(ctx, dColor, dOut, width, height, &whole, operatorFlags, whitePoint4, exposure, dState); // :192-218
}

} // extern "C"
