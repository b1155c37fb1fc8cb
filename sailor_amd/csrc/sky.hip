// The sky for gfx950: the producer of the `Sky` target and of g_skyCubemap, the sampler EnvironmentNode bakes the IBL cubes from.
//
// Replaces the GPU work of SkyNode::Process (FrameGraph/SkyNode.cpp:524-818) with Content/Shaders/Sky.shader under four define sets:
//   {FILL}    -> k_sky_march<true>   the atmosphere into the node's 256 x 256 m_pSkyTexture            (SkyNode.cpp:536-563, Sky.shader:717-734)
//   {}        -> k_sky_march<false>  the same integral into one face of g_skyCubemap, no Earth test    (SkyNode.cpp:764-797)
//   {SUN}     -> k_sky_sun           the 32 x 32 sun disk                                              (SkyNode.cpp:611-642, Sky.shader:693-715)
//   {COMPOSE} -> k_sky_compose       sky + sun over the full-resolution target                         (SkyNode.cpp:644-680, Sky.shader:613-643)
// All images are RGBA32F in device memory (the reference: R16G16B16A16_SFLOAT), row 0 = top, texel (i, j) of a w x h target has the quad's
// inTexcoord ((i + 0.5) / w, (j + 0.5) / h); the vertex shader flips y for every define set but COMPOSE (Sky.shader:90-92).  Alpha, which the
// shader leaves unwritten except under SUN, is stored as 0.
//
// Arithmetic.  tests/sky_ref.py (Ref32) restates this file operation by operation in NumPy float32 and is its specification.  The library is compiled
// with -ffp-contract=off, IEEE division and square root: every expression below is evaluated as written, with the library's conventions
// dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, mat4 * vec4 row by row left to right, length = sqrt(dot), normalize(v) = v / length(v),
// mix(a, b, t) = a (1 - t) + b t, min and max by their GLSL definitions (common.h).  Every branch of SkyLighting (outer <= 0, inner > 0, the
// discriminant sign, length(destination - origin) < 0.01, h1 < 0, theta < zeta, the sun's Earth test) is decided by geometry computed in that order
// and never by an accumulated sum.  With R = 6 371 000 in fp32, c = dot(r0, r0) - sr * sr cancels catastrophically and heights are quantised to 0.5 m:
// the fp32 result is the specification.  Only the sums over the 127 view steps (densityR, densityMie, resR, resMie) are reassociated -- they are sums
// of non-negative terms; the eight-term light sums stay sequential.
//
// Decisions where "as written" needs one (Sky.shader line numbers):
//   * exp(x) = canonical_exp2f(x * log2(e)) (canonical_math.h).  Its argument clamp to [-126, 127] replaces overflow to +inf and underflow to 0: on an
//     ENV ray that passes through the Earth (the down face) exp(-h / H0Mie) is 2^127, not inf, and the transmittance 2^-126, not 0.  Such a point
//     is under ground (h1 < 0 at j = 0), contributes nothing itself, and what lies behind it is multiplied by 2^-126.
//   * pow(v, vec3(1.5)) in PhaseMie (:198) = v * sqrt(v); pow(x, 2) (:365) = x * x.  CalculateSunColor / CalculateSunIlluminance (:247-275) are not
//     called by any of the four define sets.
//   * Rotate (Math.glsl:30-74) takes sin and cos of half of an angle of at most SunAngularR = 0.0095: the Taylor polynomials
//     x (1 + x^2 (-1/6 + x^2 / 120)) and 1 + x^2 (-1/2 + x^2 / 24), whose truncation error (x^6 / 720 < 1e-17) is far below fp32.
//   * abs(atan(y, x)) < PI / 2 in COMPOSE (:629-635) is the sign test x > 0 with x = dot(dirWorldSpace, dirToSun); atan(0, 0) is undefined in GLSL.
//   * clamp(0, 1, luminance) (:642) is GLSL's clamp(x = 0, minVal = 1, maxVal = luminance) = min(max(0, 1), luminance) = min(1, luminance).  Literal.
//   * the loop of SkyLighting does not reach the SUN result (:368 multiplies by the commented-out term): k_sky_sun does not run it.
//   * skySampler: bilinear, Repeat; sunSampler: bilinear, clamp-to-edge (sampling.h).  cloudsSampler (:710): a NULL plane is the cleared
//     m_pCloudsTexture (SkyNode.cpp:604-609), alpha = 0; a non-NULL plane is refused here -- the sun behind clouds is sailor_hip_sky_sun_clouds
//     (sky_clouds.hip), beside the cloud march that produces the plane.
//   * inverse(frame.view) is taken once on the host (sailor_host_mat4_inverse), as are origin, dirToSun, right and up, which do not vary per texel.
//
// Shape.  k_sky_march: one wave per texel, two consecutive view steps per lane (127 steps, the last half-lane idles).  A texel costs
// 127 x (2 + 16 + 3) = 2 667 exponentials on a dependent chain; a thread per texel would put 65 536 threads = one wave per SIMD on the part with
// nothing to hide that chain behind.  A wave per texel gives 65 536 waves, the geometry of a step and its eight-step light march are independent per lane,
// densityR / densityMie at a step come from one wave-wide inclusive scan of the per-lane pair sums, and six butterfly reductions finish.  No LDS.
// k_sky_sun and k_sky_compose are one texel per lane: the first is 1 024 texels of a few dozen operations, the second streams one float4 per pixel.
#include "sky_common.h"

// one view step of SkyLighting (:320-350): everything that does not need the running densities
template <bool EARTH>
__device__ __forceinline__ void sky_view_step(const S3 origin, const S3 step, const S3 sun, const float dStep, const int i, float& hr, float& hm,
                                              float& lightR, float& lightMie, bool& reached)
{
    const S3 point = sky_madd(origin, step, (float)(i + 1));
    const float h = sky_len(point) - SKY_R;
    hr = sky_exp(-h / SKY_H0R) * dStep;
    hm = sky_exp(-h / SKY_H0MIE) * dStep;
    const S3 toLight = intersect_sphere<EARTH>(point, sun);
    const float hLight = sky_len(toLight) - SKY_R;
    const float stepToLight = (hLight - h) / 8.0f;
    const float dStepLight = sky_len(sky_sub(toLight, point)) / 8.0f;
    lightR = 0.0f; lightMie = 0.0f; reached = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float h1 = h + stepToLight * (float)j;
        if (h1 < 0.0f) reached = false; // the shader breaks here and drops the step; what is summed after it is never used
        lightMie = lightMie + sky_exp(-h1 / SKY_H0MIE) * dStepLight;
        lightR = lightR + sky_exp(-h1 / SKY_H0R) * dStepLight;
    }
}

__device__ __forceinline__ float wave_inclusive_scan(float v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float t = __shfl_up(v, d, 64);
        if (lane >= d) v = v + t;
    }
    return v;
}

// ---- a. FILL and ENV: SkyLighting (:277-379) per texel, a wave per texel --------------------------------------------------------------------
template <bool EARTH>
__global__ __launch_bounds__(256) void k_sky_march(float4* __restrict__ out, int W, int H, const SkyUniforms U)
{
    const int lane = (int)(threadIdx.x & 63);
    const long long texel = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (texel >= (long long)W * H) return; // wave-uniform
    const int i = (int)(texel % W), j = (int)(texel / W);
    const float tx = ((float)i + 0.5f) / (float)W, ty = 1.0f - ((float)j + 0.5f) / (float)H;
    const S3 direction = sky_view_direction(U, tx, ty);
    const S3 origin = U.origin, sun = U.sun;

    const S3 destination = intersect_sphere<EARTH>(origin, direction);
    const S3 d = sky_sub(destination, origin);
    const float dl = sky_len(d);
    if (dl < 0.01f) { // :281-284, wave-uniform
        if (lane == 0) out[texel] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float angle = sky_dot({d.x / dl, d.y / dl, d.z / dl}, sun); // :287
    const S3 step = {d.x / 128.0f, d.y / 128.0f, d.z / 128.0f};        // :289
    const float dStep = sky_len(step);                                // :301

    float hr[2], hm[2], lR[2], lM[2];
    bool reached[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int s = 2 * lane + k;
        sky_view_step<EARTH>(origin, step, sun, dStep, s, hr[k], hm[k], lR[k], lM[k], reached[k]);
        if (s >= SKY_STEPS) { hr[k] = 0.0f; hm[k] = 0.0f; reached[k] = false; }
    }
    // densityR / densityMie after step s = the sum of hr / hm over steps 0 .. s (:326-327)
    const float inclR = wave_inclusive_scan(hr[0] + hr[1], lane), inclM = wave_inclusive_scan(hm[0] + hm[1], lane);
    float beforeR = __shfl_up(inclR, 1, 64), beforeM = __shfl_up(inclM, 1, 64);
    if (lane == 0) { beforeR = 0.0f; beforeM = 0.0f; }

    const float b0r[3] = {3.8e-6f, 13.5e-6f, 33.1e-6f}; // :292
    const float b0mie = 22e-6f, b0mie11 = 22e-6f * 1.1f; // :296, :354
    float resR[3] = {0.0f, 0.0f, 0.0f}, resMie[3] = {0.0f, 0.0f, 0.0f};
    float densityR = beforeR, densityMie = beforeM;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        densityR = densityR + hr[k];
        densityMie = densityMie + hm[k];
        if (reached[k]) { // :352-357
            const float sumR = densityR + lR[k], sumMie = lM[k] + densityMie;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float aggr = sky_exp(-b0r[c] * sumR - b0mie11 * sumMie);
                resR[c] = resR[c] + aggr * hr[k];
                resMie[c] = resMie[c] + aggr * hm[k];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { resR[c] = wave_sum(resR[c]); resMie[c] = wave_sum(resMie[c]); }
    if (lane != 0) return;

    const float phaseR = ((3.0f * SKY_PI) / 16.0f) * (1.0f + angle * angle); // :186-189
    float phaseMie; // :193-199
    {
        const float cc[3] = {.256098f, .132268f, .010016f}, dd[3] = {-1.5f, -1.74f, -1.98f}, ee[3] = {1.5625f, 1.7569f, 1.9801f};
        float q[3];
        for (int c = 0; c < 3; c++) {
            const float den = dd[c] * angle + ee[c];
            q[c] = ((angle * angle + 1.0f) * cc[c]) / (den * sqrtf(den));
        }
        const float third = .33333333333f;
        phaseMie = (q[0] * third + q[1] * third) + q[2] * third;
    }
    float f[3];
    for (int c = 0; c < 3; c++) f[c] = 7.0f * ((b0r[c] * resR[c]) * phaseR + (b0mie * resMie[c]) * phaseMie); // :376
    out[texel] = make_float4(f[0], f[1], f[2], 0.0f);
}

// ---- b. SUN (:693-715 and the SUN branches of SkyLighting) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sky_sun(float4* __restrict__ out, int W, int H, const SkyUniforms U)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    float4* __restrict__ o = out + (size_t)j * (size_t)W + i;
    *o = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // :705
    const float tx = ((float)i + 0.5f) / (float)W, ty = 1.0f - ((float)j + 0.5f) / (float)H;
    // :710-712: the clouds plane is cleared, alpha = 0 < 0.5
    const float v = sky_sun_texel(U, tx, ty);
    *o = make_float4(v, v, v, 0.0f);
}

// ---- c. COMPOSE (:613-643) -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sky_merge(float o, float s, float t) // :642 max(out, mix(out, sun, t))
{
    const float m = o * (1.0f - t) + s * t;
    return o < m ? m : o;
}

__global__ __launch_bounds__(256) void k_sky_compose(const float4* __restrict__ sky, int SW, int SH, const float4* __restrict__ sun, int NW, int NH,
                                                     float4* __restrict__ out, int W, int H, int rowBegin, int rowCount, const SkyUniforms U)
{
    const int i = texel_i(), r = texel_j();
    if (i >= W || r >= rowCount) return;
    const int j = rowBegin + r;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const S3 dir = sky_view_direction(U, u, 1.0f - v); // :614-619
    float4 c = sample_repeat_f4(sky, SW, SH, u, v);    // :621
    c.w = 0.0f;
    const S3 rel = sky_sub(dir, U.sun);
    const float dx = sky_dot(rel, U.right), dy = sky_dot(rel, U.up); // :626-627
    if (dx > -SKY_SUN_R && dy > -SKY_SUN_R && dx < SKY_SUN_R && dy < SKY_SUN_R && sky_dot(dir, U.sun) > 0.0f) { // :631-635
        const float su = 1.0f - (dx / SKY_SUN_R + 1.0f) / 2.0f, sv = 1.0f - (dy / SKY_SUN_R + 1.0f) / 2.0f; // :637-639
        const float4 s = sample_clamp_f4(sun, NW, NH, su, sv);
        const float lum = (s.x * s.x + s.y * s.y) + s.z * s.z;
        const float t = lum < 1.0f ? lum : 1.0f; // clamp(0, 1, luminance) = min(max(0, 1), luminance)
        c.x = sky_merge(c.x, s.x, t); c.y = sky_merge(c.y, s.y, t); c.z = sky_merge(c.z, s.z, t);
    }
    out[(size_t)r * (size_t)W + i] = c;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------

// glm::rotate(glm::mat4(1), angle, axis) for a unit axis (glm/ext/matrix_transform.inl), column-major
static void sky_rotation(float angleRadians, const float* axis, float* m)
{
    const float c = cosf(angleRadians), s = sinf(angleRadians);
    const float t[3] = {(1.0f - c) * axis[0], (1.0f - c) * axis[1], (1.0f - c) * axis[2]};
    const float r[16] = {c + t[0] * axis[0], t[0] * axis[1] + s * axis[2], t[0] * axis[2] - s * axis[1], 0.0f,
                         t[1] * axis[0] - s * axis[2], c + t[1] * axis[1], t[1] * axis[2] + s * axis[0], 0.0f,
                         t[2] * axis[0] + s * axis[1], t[2] * axis[1] - s * axis[0], c + t[2] * axis[2], 0.0f,
                         0.0f, 0.0f, 0.0f, 1.0f};
    memcpy(m, r, sizeof r);
}

extern "C" {

int sailor_host_sky_params_default(SailorSkyParams* p) // SkyNode.h:50-67
{
    if (!p) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const float l = sqrtf((0.0f * 0.0f + -1.0f * -1.0f) + 1.0f * 1.0f); // normalize(vec4(0, -1, 1, 0))
    const SailorSkyParams d = {{0.0f / l, -1.0f / l, 1.0f / l, 0.0f / l}, 0.3f, 0.06f, 0.3f, 0.56f, 0.025f, 0.9f, 0.95f, 0.51f, 10.0f, 500.0f, 0.5f, 5,
                               0.5f, 0.5f, 0.5f, 0.45f, 60};
    *p = d;
    return SAILOR_HIP_OK;
}

int sailor_host_sky_face_matrices(int32_t face, float* outView16, float* outProjection16, float* outInvProjection16) // SkyNode.cpp:487-495
{
    if (face < 0 || face > 5 || !outView16 || !outProjection16 || !outInvProjection16) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const float deg = 0.01745329251994329576923690768489f; // glm::radians
    const float up[3] = {0.0f, 1.0f, 0.0f}, right[3] = {1.0f, 0.0f, 0.0f};
    float a[16], b[16];
    switch (face) {
    case 0: sky_rotation(-90.0f * deg, up, outView16); break;
    case 1: sky_rotation(90.0f * deg, up, outView16); break;
    case 2: sky_rotation(-90.0f * deg, right, a); sky_rotation(180.0f * deg, up, b); sailor_host_mat4_mul(a, b, outView16); break;
    case 3: sky_rotation(90.0f * deg, right, a); sky_rotation(180.0f * deg, up, b); sailor_host_mat4_mul(a, b, outView16); break;
    case 4: sky_rotation(180.0f * deg, up, outView16); break;
    default: sky_rotation(0.0f * deg, up, outView16); break;
    }
    int st = sailor_host_perspective_rh(90.0f * deg, 1.0f, 0.1f, 1000.0f, outProjection16);
    if (st != SAILOR_HIP_OK) return st;
    return sailor_host_mat4_inverse(outProjection16, outInvProjection16);
}

int sailor_hip_sky_fill(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params, float* dSky, int32_t width, int32_t height)
{
    if (!ctx || !frame || !params || !aligned(dSky, 16) || !extent_ok(width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SkyUniforms U;
    if (!sky_uniforms(frame->view, frame->invProjection, frame->cameraPosition, params, &U)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned blocks = (unsigned)(((long long)width * height + 3) / 4);
    sailor_launch(ctx, k_sky_march<true>, dim3(blocks), dim3(256), (float4*)dSky, (int)width, (int)height, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_march<fill>");
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_env_face(SailorHipContext* ctx, const float* cameraPosition3, const SailorSkyParams* params, float* dCube, int32_t size, int32_t face)
{
    if (!ctx || !cameraPosition3 || !params || !aligned(dCube, 16) || !extent_ok(size, size) || face < 0 || face > 5) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    float view[16], projection[16], invProjection[16];
    if (sailor_host_sky_face_matrices(face, view, projection, invProjection) != SAILOR_HIP_OK) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SkyUniforms U;
    if (!sky_uniforms(view, invProjection, cameraPosition3, params, &U)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const unsigned blocks = (unsigned)(((long long)size * size + 3) / 4);
    sailor_launch(ctx, k_sky_march<false>, dim3(blocks), dim3(256), (float4*)dCube + (size_t)face * size * size, (int)size, (int)size, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_march<env>");
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_sun(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params, const float* dClouds, int32_t cloudsWidth,
                       int32_t cloudsHeight, float* dSun, int32_t width, int32_t height)
{
    if (!ctx || !frame || !params || !aligned(dSun, 16) || !extent_ok(width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    (void)cloudsWidth; (void)cloudsHeight;
    if (dClouds) { ctx->lastError = "sailor_hip_sky_sun: a clouds plane is taken by sailor_hip_sky_sun_clouds"; return SAILOR_HIP_ERR_UNSUPPORTED; }
    SkyUniforms U;
    if (!sky_uniforms(frame->view, frame->invProjection, frame->cameraPosition, params, &U)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_sun, texel_grid(width, height), dim3(256), (float4*)dSun, (int)width, (int)height, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_sun");
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_compose(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params, const float* dSky, int32_t skyWidth,
                           int32_t skyHeight, const float* dSun, int32_t sunWidth, int32_t sunHeight, float* dOut, int32_t width, int32_t height,
                           const SailorBand* band)
{
    if (!ctx || !frame || !params || !band || !extent_ok(width, height) || !extent_ok(skyWidth, skyHeight) || !extent_ok(sunWidth, sunHeight))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!sailor_hip_band_is_valid(width, height, band)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!aligned(dSky, 16) || !aligned(dSun, 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!band->fbRowCount) return SAILOR_HIP_OK; // a rank without rows holds no target
    if (!aligned(dOut, 16) || dOut == dSky || dOut == dSun) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SkyUniforms U;
    if (!sky_uniforms(frame->view, frame->invProjection, frame->cameraPosition, params, &U)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_compose, texel_grid(width, band->fbRowCount), dim3(256), (const float4*)dSky, (int)skyWidth, (int)skyHeight, (const float4*)dSun,
                  (int)sunWidth, (int)sunHeight, (float4*)dOut, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_compose");
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_env_cubemap(SailorHipContext* ctx, const float* cameraPosition3, const SailorSkyParams* params, float* dCube, int32_t size, int32_t levels)
{
    // every argument is checked before the first launch (the mip generator's own limits included): a refused call records nothing
    if (!ctx || !cameraPosition3 || !params || !aligned(dCube, 16) || size <= 0 || size > 8192 || levels <= 0 || levels > 16) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    for (int32_t face = 0; face < 6; face++) { // SkyNode.cpp:768-797, one face per frame there
        const int st = sailor_hip_sky_env_face(ctx, cameraPosition3, params, dCube, size, face);
        if (st != SAILOR_HIP_OK) return st;
    }
    return sailor_hip_generate_mipmaps_cube(ctx, dCube, size, levels); // :800-801
}

} // extern "C"
