// Horizon-based ambient occlusion for gfx950: the producer of the g_AO target that Standard.shader:386 reads.
//
// Replaces the GPU work of five consecutive nodes of the shipped frame graph (tests/golden/DefaultRenderer.renderer:202-264), of which
// DepthHighZ already has its entry points (sailor_hip_hiz_*):
//   * Blit DepthBuffer -> HalfDepth (FrameGraph/BlitNode.cpp:21-124; depth formats are blitted with Nearest, :88)  -> k_blit_nearest
//   * PostProcess with Content/Shaders/HBAO.shader:81-249 -> AO                                                     -> k_hbao
//   * PostProcess twice with Content/Shaders/HBAO_Blur.shader:67-111 (VERTICAL -> TemporaryR8, HORIZONTAL -> g_AO)  -> k_hbao_blur<VERTICAL>
// All images are single-channel fp32 planes, row 0 = top; texel (i, j) of a w x h target has fragTexcoord = ((i + 0.5) / w, (j + 0.5) / h).
// The R8_UNORM targets are kept as fp32 planes that hold what a later texture() of the 8-bit target would return (store_unorm8 below).
//
// Arithmetic is evaluated exactly as the shaders write it, in their order, one IEEE rounding per operation (-ffp-contract=off, IEEE division and
// square root, denormals kept); tests/hbao_ref.py restates it in NumPy float32 and the kernels reproduce it bit for bit.  Where GLSL fixes no order
// this file uses the library's: dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, mat4 * vec4 row by row left to right, v / s = one division per
// component, length = sqrt(dot), normalize(v) = v / length(v), rcp(x) = 1 / x, mix(a, b, t) = a (1 - t) + b t, products left to right.
//
// Decisions where "as written" needs one (HBAO.shader line numbers):
//   * main() normalises the normal a second time (:199 around :116): both are kept.
//   * ClipSpaceToViewSpace is fed (uv.x, uv.y, depth, 1) -- texture coordinates, not NDC (:91, :112-114).  Literal.
//   * depthSampler / aoSampler: bilinear, clamp-to-edge = sample_clamp_f1 of sampling.h.  SnapTexel puts most sample points on texel corners, but
//     (k * (1 / W)) * W is not always k in fp32, so the weights are not always one half: the four taps are evaluated, there is no "corner depth" plane.
//   * noiseSampler: nearest, repeat (Content/Textures/Noise.png.asset:5-6): texel floor(u * nw) mod nw of the caller's decoded linear float4 texels.
//   * round() of SnapTexel is round-half-to-even (rintf = v_rndne_f32); GLSL leaves the tie open.
//   * screenSpace1Meter (:211) projects the view-space point (0, 1, 0, 1): clip w = 0, x = 0 / 0 = NaN for every perspective projection, so maxAORadius
//     is NaN and min(x, y) = "y < x ? y : x" returns data.occlusionRadius: sampleRadius = occlusionRadius.  The else branch (:215-219) is dead.
//   * sinS = sin(PI / 2 - acos(x)) (:133) is x; implemented as x (no clamp: a NaN stays NaN and fails both comparisons of :135).  acos' GLSL precision
//     is far wider than the difference, and the pass then has no transcendental function at all.  tests/hbao_ref.py's float64 form keeps sin / acos.
//   * saturate(x) = glsl_saturate of common.h: a NaN passes through and becomes 0 only in the final store.
//   * hostile depth (0, inf, NaN) makes sample coordinates non-finite; the float -> int conversion of the tap computation is then the saturating one
//     with NaN -> 0 (what v_cvt_i32_f32 does), spelled out in bilinear_taps_saturating of sampling.h instead of left to an undefined C++ cast
//     (sampling.h's header says why the library has both).
//   * the sky check (:190-194) and screenSpaceRadius < 1 (:225) store 1; distanceFactor (:138) is not clamped and may be negative.
//   * only .r of the targets exists.
//
// Shape.  One AO texel per lane, 256-thread blocks of 64 x 4 texels: the 70 depth fetches of a texel are 4 gathers each from a plane that fits the
// L2 (HalfDepth at 4K is 14.7 MB), neighbouring lanes march neighbouring rays, and nothing is shared between lanes, so no LDS and no barrier.
// The eight directions are a rolled loop (the ordered sum over directions and the carried sinH of a ray stay in one lane).
// The blur is one destination texel per lane as well: 2 + 4 * radius bilinear fetches, of which the AO taps hit the cache.
#include "common.h"
#include "sampling.h"
#include "texel_pass.h"
#include "canonical_math.h"
#include <math.h>

// what texture() returns from an R8_UNORM target after v was written to it; NaN -> 0
__device__ __forceinline__ float store_unorm8(float v)
{
    const float c = v != v ? 0.0f : (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v));
    return rintf(c * 255.0f) / 255.0f;
}

// ---- a. nearest down-scaling blit -------------------------------------------------------------------------------------------------------
// the source texel that contains the destination texel's centre: ((2 i + 1) srcW) / (2 dstW) in integers
__global__ __launch_bounds__(256) void k_blit_nearest(const float* __restrict__ src, int srcW, int srcH, float* __restrict__ dst, int dstW, int dstH)
{
    const int i = texel_i(), j = texel_j();
    if (i >= dstW || j >= dstH) return;
    const int sx = (int)(((long long)(2 * (long long)i + 1) * srcW) / (2 * (long long)dstW));
    const int sy = (int)(((long long)(2 * (long long)j + 1) * srcH) / (2 * (long long)dstH));
    dst[(size_t)j * (size_t)dstW + i] = src[(size_t)sy * (size_t)srcW + sx];
}

// ---- b. the HBAO pass -------------------------------------------------------------------------------------------------------------------
struct HbaoArgs {
    Mat4 invProjection;
    float zNear;
    float viewportH; // float(frame.viewportSize.y)
    SailorHbaoParams p;
};

struct V3 { float x, y, z; };

// Math.glsl:143-154 ClipSpaceToViewSpace(vec4(u, v, depth, 1), invProjection).xyz
__device__ __forceinline__ V3 clip_to_view(const Mat4& M, float u, float v, float depth)
{
    const float4 c = glsl_mul(M, u, v, depth, 1.0f);
    V3 r;
    r.x = c.x / c.w; r.y = c.y / c.w; r.z = -(c.z / c.w);
    return r;
}

__device__ __forceinline__ float smaller_abs_delta(float left, float mid, float right) // HBAO.shader:81-86
{
    const float a = mid - left, b = right - mid;
    return fabsf(a) < fabsf(b) ? a : b;
}

__device__ __forceinline__ V3 normalize3(V3 v)
{
    const float l = sqrtf(dot3f(v.x, v.y, v.z, v.x, v.y, v.z));
    V3 r;
    r.x = v.x / l; r.y = v.y / l; r.z = v.z / l;
    return r;
}

__device__ __forceinline__ float snap_texel(float x, float size, float invSize) { return rintf(x * size) * invSize; } // :119-122

__constant__ float c_hbaoDirections[16] = { // :69-79
    0.0f, 1.0f, 1.0f, 0.0f, 0.0f, -1.0f, -1.0f, 0.0f, -0.7071069f, 0.7071068f, 0.7071068f, 0.7071069f, 0.7071069f, -0.7071068f, -0.7071068f, -0.7071069f};

__global__ __launch_bounds__(256) void k_hbao(const float* __restrict__ depth, int DW, int DH, const float4* __restrict__ noise, int NW, int NH,
                                              float* __restrict__ ao, int W, int H, const HbaoArgs A)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    float* __restrict__ out = ao + (size_t)j * (size_t)W + i;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const float sizeX = (float)DW, sizeY = (float)DH;     // :196 depthTextureSize
    const float invX = 1.0f / sizeX, invY = 1.0f / sizeY; // rcp(depthTextureSize)

    const float d = sample_clamp_f1(depth, DW, DH, u, v);
    V3 P = clip_to_view(A.invProjection, u, v, d); // :187
    if (P.z > 49000.0f) { *out = store_unorm8(1.0f); return; } // :190-194

    V3 N;
    { // :94-117 GetViewSpaceNormal, then :199
        const float uL = u + -1.0f * invX, uR = u + 1.0f * invX, vD = v + -1.0f * invY, vU = v + 1.0f * invY;
        const float dL = sample_clamp_f1(depth, DW, DH, uL, v), dR = sample_clamp_f1(depth, DW, DH, uR, v);
        const float dD = sample_clamp_f1(depth, DW, DH, u, vD), dU = sample_clamp_f1(depth, DW, DH, u, vU);
        const float ddx = smaller_abs_delta(dL, d, dR), ddy = smaller_abs_delta(dD, d, dU);
        const V3 r = clip_to_view(A.invProjection, uR, v, d + ddx), t = clip_to_view(A.invProjection, u, vU, d + ddy);
        const V3 right = {r.x - P.x, r.y - P.y, r.z - P.z}, up = {t.x - P.x, t.y - P.y, t.z - P.z};
        const V3 c = {up.y * right.z - right.y * up.z, up.z * right.x - right.z * up.x, up.x * right.y - right.x * up.y}; // cross(up, right)
        N = normalize3(normalize3(c));
    }
    { // :201
        const float s = 1.0f + (0.1f * P.z) / A.zNear;
        P.x = P.x + (N.x * 0.00001f) * s; P.y = P.y + (N.y * 0.00001f) * s; P.z = P.z + (N.z * 0.00001f) * s;
    }
    float4 nz;
    { // :203 nearest, repeat
        const int kx = cvt_i32_saturating(floorf((u * A.p.noiseScale) * (float)NW)), ky = cvt_i32_saturating(floorf((v * A.p.noiseScale) * (float)NH));
        const int tx = wrap_tap(kx, NW), ty = wrap_tap(ky, NH);
        nz = noise[(size_t)ty * NW + tx];
    }
    const float offX = (nz.x * 2.0f - 1.0f) / 4.0f, offY = (nz.y * 2.0f - 1.0f) / 4.0f; // :204
    const float jitter = nz.y;

    // :206-214: maxAORadius is NaN for every perspective projection (header comment), so min() returns its first argument
    const float sampleRadius = A.p.occlusionRadius;
    const float resolutionRatio = sizeY / A.viewportH;                            // :222
    const float screenSpaceRadius = ((50.0f * sampleRadius) * resolutionRatio) / P.z; // :223
    if (screenSpaceRadius < 1.0f) { *out = store_unorm8(1.0f); return; }              // :225-229

    const float radX = screenSpaceRadius * invX, radY = screenSpaceRadius * invY; // :241
    const float R2 = A.p.occlusionRadius * A.p.occlusionRadius;
    const float invR2 = 1.0f / R2, invAtt = 1.0f / A.p.occlusionAttenuation;
    const float bias3 = A.p.occlusionBias * 3.0f;
    const float inv9 = 1.0f / 9.0f; // rcp(NumSamples + 1.0f)

    float occlusionFactor = 0.0f;
#pragma unroll 1
    for (int k = 0; k < 8; k++) { // :234-245
        float dirX = c_hbaoDirections[2 * k] + offX, dirY = c_hbaoDirections[2 * k + 1] + offY;
        const float dl = sqrtf(dirX * dirX + dirY * dirY);
        dirX = dirX / dl; dirY = dirY / dl; // :236
        // :147-183 SampleRayAO
        const float stepTexelX = dirX * invX, stepTexelY = dirY * invY; // :158
        dirX = dirX * radX; dirY = dirY * radY;                         // :159
        const float stepX = snap_texel(dirX * inv9, sizeX, invX), stepY = snap_texel(dirY * inv9, sizeY, invY); // :162
        const float jitX = stepTexelX * (1.0f - jitter) + stepX * jitter, jitY = stepTexelY * (1.0f - jitter) + stepY * jitter; // :163
        const float startX = snap_texel(u + jitX, sizeX, invX), startY = snap_texel(v + jitY, sizeY, invY); // :164
        const float endX = startX + dirX, endY = startY + dirY; // :165
        float occlusion = 0.0f;
        float sinH = A.p.occlusionBias;
#pragma unroll
        for (int s = 0; s < 8; s++) { // :174-180
            const float t = (float)s / 8.0f;
            const float su = snap_texel(startX * (1.0f - t) + endX * t, sizeX, invX), sv = snap_texel(startY * (1.0f - t) + endY * t, sizeY, invY);
            const V3 S = clip_to_view(A.invProjection, su, sv, sample_clamp_f1(depth, DW, DH, su, sv));
            // :124-145 SampleAO
            const V3 hv = {S.x - P.x, S.y - P.y, S.z - P.z};
            const float len = sqrtf(dot3f(hv.x, hv.y, hv.z, hv.x, hv.y, hv.z));
            const float sinS = dot3f(N.x, N.y, N.z, hv.x / len, hv.y / len, hv.z / len); // :133
            float occ = 0.0f;
            if (len < R2 && sinS > sinH + bias3) { // :135
                const float falloffZ = 1.0f - glsl_saturate(fabsf(hv.z) * 0.007f);
                const float distanceFactor = 1.0f - (len * invR2) * invAtt;
                occ = ((sinS - sinH) * distanceFactor) * falloffZ;
                sinH = sinS;
            }
            occlusion = occlusion + occ;
        }
        occlusionFactor = occlusionFactor + occlusion;
    }
    *out = store_unorm8(1.0f - glsl_saturate((A.p.occlusionPower / 8.0f) * occlusionFactor)); // :247
}

// ---- c. the bilateral blur pass ---------------------------------------------------------------------------------------------------------
template <bool VERTICAL>
__global__ __launch_bounds__(256) void k_hbao_blur(const float* __restrict__ ao, int AW, int AH, const float* __restrict__ depth, int DW, int DH,
                                                   float* __restrict__ dst, int W, int H, const SailorHbaoBlurParams p)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const float pixX = VERTICAL ? 0.0f : 1.0f / (float)DW, pixY = VERTICAL ? 1.0f / (float)DH : 0.0f; // HBAO_Blur.shader:84-90
    const float centerD = sample_clamp_f1(depth, DW, DH, u, v);
    float totalC = sample_clamp_f1(ao, AW, AH, u, v), totalW = 1.0f; // :92-96
    const float sigma = p.radius * p.sharpness;                      // :72
    const float falloff = 1.0f / ((2.0f * sigma) * sigma);           // :73
    for (int side = 0; side < 2; side++) // :98-108: all + taps, then all - taps
        for (float r = 1.0f; r <= p.radius; r += 1.0f) {
            const float su = side ? u - pixX * r : u + pixX * r, sv = side ? v - pixY * r : v + pixY * r;
            const float c = sample_clamp_f1(ao, AW, AH, su, sv), d = sample_clamp_f1(depth, DW, DH, su, sv); // :69-70
            const float diff = (d - centerD) * p.distanceScale;                                        // :75
            const float w = canonical_exp2f(((-r * r) * falloff) - diff * diff);                       // :76
            totalW = totalW + w;
            totalC = totalC + c * w;
        }
    dst[(size_t)j * (size_t)W + i] = store_unorm8(totalC / totalW); // :110
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------
#define HBAO_MAX_BLUR_RADIUS 64.0f

static bool blit_args_ok(SailorHipContext* ctx, const float* s, int32_t sw, int32_t sh, float* d, int32_t dw, int32_t dh)
{
    return ctx && s && d && s != d && extent_ok(sw, sh) && extent_ok(dw, dh);
}
static bool hbao_args_ok(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* d, int32_t dw, int32_t dh, const float* n, int32_t nw, int32_t nh,
                         const SailorHbaoParams* p, float* ao, int32_t w, int32_t h)
{
    return ctx && frame && d && p && ao && d != ao && aligned(n, 16) && extent_ok(dw, dh) && extent_ok(nw, nh) && extent_ok(w, h);
}
static bool blur_args_ok(SailorHipContext* ctx, const float* a, int32_t aw, int32_t ah, const float* d, int32_t dw, int32_t dh, const SailorHbaoBlurParams* p,
                         float* o, int32_t w, int32_t h)
{
    // the loop count is data.radius: a NaN runs no tap, anything above the cap is refused rather than run for seconds
    return ctx && a && d && p && o && a != o && d != o && extent_ok(aw, ah) && extent_ok(dw, dh) && extent_ok(w, h) && !(p->radius > HBAO_MAX_BLUR_RADIUS);
}

extern "C" {

int sailor_hip_blit_nearest(SailorHipContext* ctx, const float* dSrc, int32_t srcWidth, int32_t srcHeight, float* dDst, int32_t dstWidth, int32_t dstHeight)
{
    if (!blit_args_ok(ctx, dSrc, srcWidth, srcHeight, dDst, dstWidth, dstHeight)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_blit_nearest, texel_grid(dstWidth, dstHeight), dim3(256), dSrc, (int)srcWidth, (int)srcHeight, dDst, (int)dstWidth, (int)dstHeight);
    SAILOR_CHECK_LAUNCH(ctx, "k_blit_nearest");
    return SAILOR_HIP_OK;
}

int sailor_hip_hbao(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* dDepth, int32_t depthWidth, int32_t depthHeight,
                    const float* dNoise, int32_t noiseWidth, int32_t noiseHeight, const SailorHbaoParams* params, float* dAo, int32_t width, int32_t height)
{
    if (!hbao_args_ok(ctx, frame, dDepth, depthWidth, depthHeight, dNoise, noiseWidth, noiseHeight, params, dAo, width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    HbaoArgs A;
    memcpy(A.invProjection.m, frame->invProjection, sizeof A.invProjection.m);
    A.zNear = frame->cameraZNearZFar[0];
    A.viewportH = (float)frame->viewportSize[1];
    A.p = *params;
    sailor_launch(ctx, k_hbao, texel_grid(width, height), dim3(256), dDepth, (int)depthWidth, (int)depthHeight, (const float4*)dNoise, (int)noiseWidth, (int)noiseHeight,
                  dAo, (int)width, (int)height, A);
    SAILOR_CHECK_LAUNCH(ctx, "k_hbao");
    return SAILOR_HIP_OK;
}

int sailor_hip_hbao_blur_pass(SailorHipContext* ctx, const float* dAo, int32_t aoWidth, int32_t aoHeight, const float* dDepth, int32_t depthWidth, int32_t depthHeight,
                              const SailorHbaoBlurParams* params, float* dDst, int32_t width, int32_t height, int32_t vertical)
{
    if (!blur_args_ok(ctx, dAo, aoWidth, aoHeight, dDepth, depthWidth, depthHeight, params, dDst, width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    if (vertical)
        sailor_launch(ctx, k_hbao_blur<true>, texel_grid(width, height), dim3(256), dAo, (int)aoWidth, (int)aoHeight, dDepth, (int)depthWidth, (int)depthHeight, dDst,
                      (int)width, (int)height, *params);
    else
        sailor_launch(ctx, k_hbao_blur<false>, texel_grid(width, height), dim3(256), dAo, (int)aoWidth, (int)aoHeight, dDepth, (int)depthWidth, (int)depthHeight, dDst,
                      (int)width, (int)height, *params);
    SAILOR_CHECK_LAUNCH(ctx, "k_hbao_blur");
    return SAILOR_HIP_OK;
}

int sailor_hip_hbao_chain(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* dDepth, int32_t depthWidth, int32_t depthHeight,
                          float* dHalfDepth, int32_t halfWidth, int32_t halfHeight, const float* dNoise, int32_t noiseWidth, int32_t noiseHeight,
                          const SailorHbaoParams* params, float* dAo, int32_t aoWidth, int32_t aoHeight, const SailorHbaoBlurParams* blurParams,
                          float* dTemp, int32_t tempWidth, int32_t tempHeight, float* dOut, int32_t outWidth, int32_t outHeight)
{
    // every argument is checked before the first launch: a refused call records nothing
    if (!blit_args_ok(ctx, dDepth, depthWidth, depthHeight, dHalfDepth, halfWidth, halfHeight) ||
        !hbao_args_ok(ctx, frame, dHalfDepth, halfWidth, halfHeight, dNoise, noiseWidth, noiseHeight, params, dAo, aoWidth, aoHeight) ||
        !blur_args_ok(ctx, dAo, aoWidth, aoHeight, dDepth, depthWidth, depthHeight, blurParams, dTemp, tempWidth, tempHeight) ||
        !blur_args_ok(ctx, dTemp, tempWidth, tempHeight, dDepth, depthWidth, depthHeight, blurParams, dOut, outWidth, outHeight) || dOut == dAo || dOut == dHalfDepth ||
        dTemp == dHalfDepth)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    int st = sailor_hip_blit_nearest(ctx, dDepth, depthWidth, depthHeight, dHalfDepth, halfWidth, halfHeight);                                   // :204-208
    if (st != SAILOR_HIP_OK) return st;
    st = sailor_hip_hbao(ctx, frame, dHalfDepth, halfWidth, halfHeight, dNoise, noiseWidth, noiseHeight, params, dAo, aoWidth, aoHeight);     // :220-234
    if (st != SAILOR_HIP_OK) return st;
    st = sailor_hip_hbao_blur_pass(ctx, dAo, aoWidth, aoHeight, dDepth, depthWidth, depthHeight, blurParams, dTemp, tempWidth, tempHeight, 1); // :237-249
    if (st != SAILOR_HIP_OK) return st;
    return sailor_hip_hbao_blur_pass(ctx, dTemp, tempWidth, tempHeight, dDepth, depthWidth, depthHeight, blurParams, dOut, outWidth, outHeight, 0); // :252-264
}

} // extern "C"
