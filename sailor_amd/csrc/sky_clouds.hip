// The clouds of the Sky node for gfx950: the half-resolution cloud march, the sun behind clouds and the blit of the clouds over the `Sky` target.
//
// Replaces the GPU work SkyNode::Process does with m_cloudsDensity > 0 (FrameGraph/SkyNode.cpp:565-731):
//   {CLOUDS}     -> k_sky_clouds       Content/Shaders/Sky.shader:386-595, :656-692 into m_pCloudsTexture        (SkyNode.cpp:565-603)
//   {SUN}        -> k_sky_sun_clouds   the sun disk with the fetch of the clouds' alpha honoured (:707-715)      (SkyNode.cpp:611-642)
//   Blit.shader  -> k_sky_blit_clouds  the clouds over the target under the AlphaBlending state                  (SkyNode.cpp:722-731)
// Images are RGBA32F in device memory as in sky.hip; texel (i, j) of a w x h target has the quad's inTexcoord ((i + 0.5) / w, (j + 0.5) / h).
// tests/clouds_ref.py (Ref32) restates this file operation by operation in NumPy float32 and is its specification; the conventions are those
// sky.hip's header lists (no contraction, dot = (x x + y y) + z z, IEEE division and square root, exp(x) = canonical_exp2f(x * log2(e)),
// min, max and clamp(x, 0, 1) by their GLSL definitions (common.h), mix(a, b, t) = a (1 - t) + b t).
//
// Decisions (Sky.shader line numbers):
//   Quirks restated, not repaired
//   * length(position.y) (:389) is |position.y|: the height of a sample is taken from y alone, not from the distance to the Earth's centre.
//   * pow(x, 1) (:399-400) is x.
//   * maxTraceDistance (:686) is the raw linearDepth, in the depth buffer's units, compared against metres; abs(linearDepth - zFar) < 1 selects
//     BigDistance.
//   * traceEnd / finalTrace (:452-494, :519) are never read: only traceStart is computed.
//   * Remap (:381-384) = newMin + ((value - min) / (max - min)) * (newMax - newMin); where min = newMin = 0 and newMax = 1 the exact identities
//     x - 0 = x, x * 1 = x, 0 + x = x are applied, and 1 + q * (0 - 1) is 1 - q (exact).  0.07, 0.15, 0.35 and 1 - 0.9 are fp32 constants.
//   Powers
//   * pow(v, 1.5) in PhaseHenyeyGreenstein (:215) is v * sqrt(v), as in PhaseMie.  4.0f * 3.1415f * pow(..) is (4 * 3.1415) * pow(..).
//   * pow(scatteringX, j) (:514-516) is the running product, dA[0] = dB[0] = dC[0] = 1.
//   * CalculateSunColor (:247-264): pow(x, 0.5) = sqrt(x), pow(x, 3) = (x * x) * x; sqrt of a negative is NaN, and clamp(NaN, 0, 1) is NaN under the
//     conventions above -- on that side of `border` the other arm of the ?: is taken, so the NaN never reaches the colour.
//   Host-side constants
//   * sunColor does not vary per texel: sailor_host_sky_sun_color computes it once in fp32.  origin, dirToSun, inverse(view), projection * view (SUN,
//     :707, sailor_host_mat4_mul) and the three time shifts of CloudsSampleDensity (:394-397: (vec * currentTime) * factor, left to right) likewise.
//   * scatteringSteps outside 0 .. 10 is refused: dA, dB, dC are float[10].
//   Samplers (sampling.h)
//   * cloudsNoiseLowSampler / cloudsNoiseHighSampler: R8_UNORM volumes, x fastest, trilinear, Repeat, the base level only -- the implicit LOD of
//     texture() inside a loop with non-uniform exits is undefined, so the mips the node allocates are never read.  cloudsMapSampler: RGBA8, bilinear,
//     Repeat.  A texel decodes as float(byte) / 255.0f.  The volumes stay bytes in memory.
//   * g_noiseSampler (:552): nearest, Repeat, texel floor(u * n) mod n, over decoded fp32 texels.  skySampler: bilinear, Repeat, as in COMPOSE.
//     linearDepth (:656): nearest, one float per texel.  cloudsSampler (SUN :710, and the blit's colorSampler): bilinear, clamp-to-edge.
//   * every tap index is wrapped or clamped into its image after the saturating float -> int conversion and without an addition that can overflow:
//     no coordinate, however large or non-finite, produces a fetch outside a plane.
//   Orientation
//   * the vertex shader flips y for CLOUDS and SUN, not for Blit.shader (:90-92): fragTexcoord = (u, 1 - v).  The CLOUDS fragment un-flips uv for
//     the view direction (uv.y = 1 - (1 - v), computed so) but samples skySampler and linearDepth at the flipped fragTexcoord (:656-671).  Literally
//     restated: ROW h - 1 OF THE CLOUDS PLANE IS THE TOP OF THE VIEW, row 0 its bottom, and the blit, which does not flip, puts row 0 on the target's
//     top row.
//   * dirWorldSpace is normalised as a vec4 (:669) and its xyz normalised again (:677): both are done.
//   SUN
//   * uvView = ((projection * view) * vec4(dir, 0) + 1) * 0.5, then all of it divided by its own w (:707-708).  Under a perspective projection the
//     clip w of a unit direction is minus its view-space z, in [-1, 1], so w lies in [0, 1]: a sun behind the camera gives a small w and coordinates far
//     outside [0, 1], clamped to the edge like any other.  w = 0 (the sun exactly behind) gives +-inf or NaN coordinates, whose bilinear weights are NaN:
//     the alpha is NaN, `clouds < 0.5` is false and the texel stays (0, 0, 0, 0).  A negative w (another projection) gives finite mirrored coordinates.
//   Blend (VulkanPipileneStates.cpp:245-246)
//   * rgb = src.rgb * src.a + dst.rgb * (1 - src.a);  a = src.a * src.a - dst.a * (1 - src.a) (the alpha op is SUBTRACT).  In place on the target.
//   Output
//   * alpha = 1 - transmittanceLow; a ray that returns early (:463-466, :500-503) still gets sky * ambient mixed by `horizon`, and alpha 0.
//   * colorLow is a vec3 whose components are equal: one float.
//
// Shape.  k_sky_clouds: a texel per lane, a wave covers an 8 x 8 tile and a block of 256 a 16 x 16 tile, so that the lanes of a wave look through
// neighbouring parts of the weather map and leave the march at similar steps.  Per texel and scattering octave j the two Henyey-Greenstein terms
// depend on mu alone: they are computed once before the march and kept in LDS (10 x 256 floats, column = thread, conflict-free), because an
// array indexed by the loop counter would otherwise live in scratch.  No scratch, no spills.  The spread of a dense step's scatteringSteps x 4
// sun-ward samples over several lanes was not built; DESIGN.md section 4 says so.
#include "sky_common.h"

#define CLOUDS_START_R 6378000.0f      // R + 7000 (:163), exact in fp32
#define CLOUDS_END_R 6393000.0f        // CloudsStartR + 15000 (:164)
#define CLOUDS_BIG_DISTANCE 600000.0f  // :496, :685
#define CLOUDS_STEPS 384               // StepsHighDetail + StepsLowDetail (:520-521)
#define CLOUDS_MAX_SCATTERING 10       // float dA[10] (:508)

struct CloudsUniforms {
    SkyUniforms sky;
    SailorSkyParams p;
    S3 sunColor;          // CalculateSunColor(-dirToSun) (:505)
    float windX, windZ;   // (vec2(0.1, 0.05) * currentTime) * 1000 (:394)
    S3 shift1, shift2;    // :396-397
    float zFar;
};

struct CloudsTextures {
    const uint32_t* __restrict__ weather; int mapW, mapH;
    const uint8_t* __restrict__ low; int lowN;
    const uint8_t* __restrict__ high; int highN;
};

// CloudsSampleDensity (:392-425)
__device__ __forceinline__ float clouds_density(const CloudsUniforms& U, const CloudsTextures& T, S3 position)
{
    const float px = position.x + U.windX, py = position.y, pz = position.z + U.windZ;
    const float cloudsLow = trilinear_repeat_r8(T.low, T.lowN, U.shift1.x + px / 9000.0f, U.shift1.y + py / 9000.0f, U.shift1.z + pz / 9000.0f);
    const float cloudsHigh = trilinear_repeat_r8(T.high, T.highN, U.shift2.x + px / 1300.0f, U.shift2.y + py / 1300.0f, U.shift2.z + pz / 1300.0f);
    const float4 weather = bilinear_repeat_rgba8(T.weather, T.mapW, T.mapH, px / 409600.0f + 0.2f, pz / 409600.0f + 0.1f);
    const float height = glsl_saturate((fabsf(py) - CLOUDS_START_R) / (CLOUDS_END_R - CLOUDS_START_R)); // :389
    const float SRb = glsl_saturate(height / 0.07f);
    const float wb35 = weather.z * 0.35f;
    const float SRt = glsl_saturate(1.0f - (height - wb35) / (weather.z - wb35));
    const float SA = SRb * SRt;
    const float DRb = height * glsl_saturate(height / 0.15f);
    const float DRt = height * glsl_saturate(1.0f - (height - 0.9f) / (1.0f - 0.9f));
    const float DA = (((DRb * DRt) * weather.w) * 2.0f) * U.p.cloudsDensity;
    const float SNsample = cloudsLow * 0.85f + cloudsHigh * 0.15f;
    const float WMc = glsl_max(weather.x, (glsl_saturate(U.p.cloudsCoverage - 0.5f) * weather.y) * 2.0f);
    const float lo = 1.0f - U.p.cloudsCoverage * WMc;
    return glsl_saturate((SNsample * SA - lo) / (1.0f - lo)) * DA;
}

// CloudsSampleDirectDensity (:427-448)
__device__ __forceinline__ float clouds_direct_density(const CloudsUniforms& U, const CloudsTextures& T, S3 position)
{
    const float avrStep = (CLOUDS_END_R - CLOUDS_START_R) * 0.01f;
    float sumDensity = 0.0f;
#pragma unroll 1
    for (int i = 0; i < 4; i++) {
        const float step = i == 3 ? avrStep * 6.0f : avrStep;
        position = sky_madd(position, U.sky.sun, step);
        sumDensity = sumDensity + clouds_density(U, T, position) * step;
    }
    return sumDensity;
}

// PhaseHenyeyGreenstein (:212-216)
__device__ __forceinline__ float clouds_phase_hg(float a, float g)
{
    const float g2 = g * g;
    const float den = (1.0f + g2) - (2.0f * g) * a;
    return (1.0f - g2) / ((4.0f * 3.1415f) * (den * sqrtf(den)));
}

// the wave's 8 x 8 tile inside the block's 16 x 16
__device__ __forceinline__ void clouds_texel(int& i, int& j)
{
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    i = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    j = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// ---- a. CLOUDS (:645-692 around CloudsMarching :450-595) ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sky_clouds(const float4* __restrict__ sky, int SW, int SH, const CloudsTextures T, const float4* __restrict__ noise,
                                                    int NW, int NH, const float* __restrict__ depth, int DW, int DH, float4* __restrict__ out, int W, int H,
                                                    const CloudsUniforms U)
{
    __shared__ float s_phase[CLOUDS_MAX_SCATTERING][256];
    int i, j;
    clouds_texel(i, j);
    if (i >= W || j >= H) return; // no barrier below: a thread only reads back its own column of s_phase
    const int tid = (int)threadIdx.x;
    const float u = ((float)i + 0.5f) / (float)W, v = 1.0f - ((float)j + 0.5f) / (float)H; // fragTexcoord (:90-92)

    const float linearDepth = fabsf(depth[(size_t)nearest_clamp(DH, v) * DW + nearest_clamp(DW, u)]); // :656
    S3 viewDir = sky_normalize(sky_view_direction(U.sky, u, 1.0f - v)); // :664-669, :677
    const float4 color = sample_repeat_f4(sky, SW, SH, u, v); // :671 (.rgb)
    const float skyTone = color.z / (1.0f + color.z); // :674-675
    float horizon = 1.0f - sky_exp(-fabsf(viewDir.y) * U.p.fog); // :680
    horizon = (horizon * horizon) * horizon;
    const S3 origin = U.sky.origin, sun = U.sky.sun;
    const float originHeight = sky_len(origin);
    horizon = horizon + (1.0f - glsl_saturate((CLOUDS_START_R - originHeight) / 500.0f)); // :682
    horizon = glsl_saturate(horizon);
    const float maxTraceDistance = fabsf(linearDepth - U.zFar) < 1.0f ? CLOUDS_BIG_DISTANCE : linearDepth; // :686

    // CloudsMarching (:450-595)
    float colorLow = 0.0f, transmittanceLow = 1.0f;
    const float2 si = ray_sphere(origin, viewDir, CLOUDS_START_R), ei = ray_sphere(origin, viewDir, CLOUDS_END_R);
    const float shiftStart = si.x < 0.0f ? glsl_max(0.0f, si.y) : si.x;
    const float shiftEnd = glsl_min(maxTraceDistance, ei.x < 0.0f ? glsl_max(0.0f, ei.y) : ei.x);
    const bool early = (shiftStart > shiftEnd && ei.x < 0.0f) || shiftStart > CLOUDS_BIG_DISTANCE; // :463-466, :500-503
    if (!early) {
        S3 traceStart = origin; // :468-494
        if (originHeight < CLOUDS_START_R) traceStart = sky_madd(origin, viewDir, shiftStart);
        else if (originHeight > CLOUDS_END_R) traceStart = sky_madd(origin, viewDir, shiftEnd);
        const float mu = glsl_max(0.0f, sky_dot(viewDir, sun)); // :506
        const int steps = U.p.scatteringSteps;
        {
            float dB = 1.0f, dC = 1.0f; // :512-517
            for (int k = 0; k < steps; k++) {
                const float m11 = U.p.phaseInfluence1 * clouds_phase_hg(mu, dC * U.p.eccentrisy1); // :559-560
                const float m12 = U.p.phaseInfluence2 * clouds_phase_hg(mu, dC * U.p.eccentrisy2);
                s_phase[k][tid] = dB * (m11 + m12); // the head of the product of :569
                dB = dB * U.p.scatteringIntensity;
                dC = dC * U.p.scatteringPhase;
            }
        }
        S3 position = traceStart;
        float avrStep = 150.0f;
#pragma unroll 1
        for (int s = 0; s < CLOUDS_STEPS; s++) {
            const float density = clouds_density(U, T, position) * avrStep;
            if (density > 0.0f) {
                float dA = 1.0f;
#pragma unroll 1
                for (int k = 0; k < steps; k++) {
                    S3 local = position;
                    if (k > 0) { // :550-553
                        const float off = (float)k / 16.0f;
                        const float4 n = noise[(size_t)nearest_repeat(NH, position.z + off) * NW + nearest_repeat(NW, position.x + off)];
                        const S3 r = sky_normalize({n.x - 0.5f, n.y - 0.5f, n.z - 0.5f});
                        local = {position.x + r.x * 10.0f, position.y + r.y * 10.0f, position.z + r.z * 10.0f};
                    }
                    const float sunDensity = clouds_direct_density(U, T, local);
                    const float kA = -dA * U.p.cloudsAttenuation1;
                    const float m2 = sky_exp(kA * sunDensity);     // :561
                    const float m3 = U.p.cloudsAttenuation2 * density; // :562
                    const float2 e = ray_sphere(local, sun, SKY_R);    // :564
                    if (glsl_max(e.x, e.y) < 0.0f) colorLow = colorLow + ((s_phase[k][tid] * m2) * m3) * transmittanceLow; // :567-570
                    transmittanceLow = transmittanceLow * sky_exp(kA * density); // :572
                    dA = dA * U.p.scatteringDensity;
                }
            }
            position = sky_madd(position, viewDir, avrStep); // :576
            const float height = sky_len(position);
            if (transmittanceLow < 0.05f || height > CLOUDS_END_R || height < CLOUDS_START_R || sky_len(sky_sub(position, traceStart)) > maxTraceDistance) break;
            if (s >= 128) avrStep = avrStep + 4.0f; // :587-590
        }
    }
    const float alpha = early ? 0.0f : 1.0f - transmittanceLow; // :593
    const float amb = skyTone * U.p.ambient;                     // :688
    float rgb[3];
    const float sc[3] = {U.sunColor.x, U.sunColor.y, U.sunColor.z}, oc[3] = {color.x, color.y, color.z};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float raw = (early ? 0.0f : (U.p.sunIntensity * sc[c]) * colorLow) + amb;
        rgb[c] = oc[c] * (1.0f - horizon) + raw * horizon; // :689
    }
    out[(size_t)j * (size_t)W + i] = make_float4(rgb[0], rgb[1], rgb[2], alpha);
}

// ---- b. SUN behind clouds (:693-715) --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sky_sun_clouds(const float4* __restrict__ clouds, int CW, int CH, float4* __restrict__ out, int W, int H,
                                                        const SkyUniforms U, const Mat4 projView)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const float tx = ((float)i + 0.5f) / (float)W, ty = 1.0f - ((float)j + 0.5f) / (float)H;
    const float ax = -SKY_SUN_R * (1.0f - tx) + SKY_SUN_R * tx, ay = -SKY_SUN_R * (1.0f - ty) + SKY_SUN_R * ty; // :696-697
    const S3 direction = sky_normalize(sky_rotate(sky_rotate(U.sun, U.up, ax), U.axis2, ay));                  // :702-703, as in sky_sun_texel
    const float4 clip = glsl_mul(projView, direction.x, direction.y, direction.z, 0.0f);                      // :707
    const float w = (clip.w + 1.0f) * 0.5f;
    const float cu = ((clip.x + 1.0f) * 0.5f) / w, cv = ((clip.y + 1.0f) * 0.5f) / w;                          // :708
    const float alpha = sample_clamp_f4(clouds, CW, CH, cu, cv).w;                                         // :710
    const float v = alpha < 0.5f ? sky_sun_texel(U, tx, ty) : 0.0f;                                           // :712-715
    out[(size_t)j * (size_t)W + i] = make_float4(v, v, v, 0.0f);
}

// ---- c. Blit Clouds (Blit.shader under EBlendMode::AlphaBlending) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sky_blit_clouds(const float4* __restrict__ clouds, int CW, int CH, float4* __restrict__ target, int W, int H,
                                                         int rowBegin, int rowCount)
{
    const int i = texel_i(), r = texel_j();
    if (i >= W || r >= rowCount) return;
    const int j = rowBegin + r;
    const float4 src = sample_clamp_f4(clouds, CW, CH, ((float)i + 0.5f) / (float)W, ((float)j + 0.5f) / (float)H);
    float4* __restrict__ t = target + (size_t)r * (size_t)W + i;
    const float4 dst = *t;
    const float k = 1.0f - src.w;
    *t = make_float4(src.x * src.w + dst.x * k, src.y * src.w + dst.y * k, src.z * src.w + dst.z * k, src.w * src.w - dst.w * k);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static void clouds_sun_color(const float* sunDirection3, float* out3) // CalculateSunColor (:247-264), fp32 as written
{
    const float zenith[3] = {0.925f, 0.861f, 0.755f}, half[3] = {0.6f, 0.4490196f, 0.1588f};
    const float ground[3] = {0.0499f * 2.0f, 0.004f * 2.0f, (4.10f * 0.00001f) * 2.0f};
    const float angle = (-sunDirection3[0] * 0.0f + -sunDirection3[1] * 1.0f) + -sunDirection3[2] * 0.0f;
    const float border = 0.1f;
    const float r1 = sqrtf((angle - border) / (1.0f - border)), r2 = angle / border;
    const float c1 = 0.0f > r1 ? 0.0f : r1, c2 = 0.0f > (r2 * r2) * r2 ? 0.0f : (r2 * r2) * r2; // max(x, 0) = x < 0 ? 0 : x
    const float t1 = 1.0f < c1 ? 1.0f : c1, t2 = 1.0f < c2 ? 1.0f : c2;
    for (int c = 0; c < 3; c++)
        out3[c] = angle > border ? half[c] * (1.0f - t1) + zenith[c] * t1 : ground[c] * (1.0f - t2) + half[c] * t2;
}

extern "C" {

int sailor_host_sky_sun_color(const float* sunDirection3, float* outColor3)
{
    if (!sunDirection3 || !outColor3) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    clouds_sun_color(sunDirection3, outColor3);
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_clouds(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params, const float* dSky, int32_t skyWidth,
                          int32_t skyHeight, const uint8_t* dWeatherMap, int32_t mapWidth, int32_t mapHeight, const uint8_t* dNoiseLow, int32_t lowSize,
                          const uint8_t* dNoiseHigh, int32_t highSize, const float* dNoise, int32_t noiseWidth, int32_t noiseHeight, const float* dLinearDepth,
                          int32_t depthWidth, int32_t depthHeight, float* dClouds, int32_t width, int32_t height)
{
    if (!ctx || !frame || !params) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!extent_ok(width, height) || !extent_ok(skyWidth, skyHeight) || !extent_ok(mapWidth, mapHeight) || !extent_ok(noiseWidth, noiseHeight) ||
        !extent_ok(depthWidth, depthHeight) || lowSize <= 0 || lowSize > 1024 || highSize <= 0 || highSize > 1024)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!aligned(dSky, 16) || !aligned(dWeatherMap, 16) || !aligned(dNoiseLow, 16) || !aligned(dNoiseHigh, 16) || !aligned(dNoise, 16) ||
        !aligned(dLinearDepth, 16) || !aligned(dClouds, 16))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if ((const void*)dClouds == dSky || (const void*)dClouds == dNoise || (const void*)dClouds == dLinearDepth || (const void*)dClouds == dWeatherMap ||
        (const void*)dClouds == dNoiseLow || (const void*)dClouds == dNoiseHigh)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (params->scatteringSteps < 0 || params->scatteringSteps > CLOUDS_MAX_SCATTERING) {
        ctx->lastError = "sailor_hip_sky_clouds: scatteringSteps outside 0 .. 10 (Sky.shader:508-510, float dA[10])";
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    }
    CloudsUniforms U;
    if (!sky_uniforms(frame->view, frame->invProjection, frame->cameraPosition, params, &U.sky)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    U.p = *params;
    const float toLight[3] = {-U.sky.sun.x, -U.sky.sun.y, -U.sky.sun.z};
    float sunColor[3];
    clouds_sun_color(toLight, sunColor);
    U.sunColor = {sunColor[0], sunColor[1], sunColor[2]};
    const float t = frame->currentTime;
    U.windX = (0.1f * t) * 1000.0f;
    U.windZ = (0.05f * t) * 1000.0f;
    U.shift1 = {(-0.0021f * t) * -0.5f, (0.0017f * t) * -0.5f, (-0.02f * t) * -0.5f};
    U.shift2 = {(0.021f * t) * -0.2f, (0.017f * t) * -0.2f, (0.0f * t) * -0.2f};
    U.zFar = frame->cameraZNearZFar[1];
    const CloudsTextures T = {(const uint32_t*)dWeatherMap, (int)mapWidth, (int)mapHeight, dNoiseLow, (int)lowSize, dNoiseHigh, (int)highSize};
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_clouds, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(256), (const float4*)dSky, (int)skyWidth,
                  (int)skyHeight, T, (const float4*)dNoise, (int)noiseWidth, (int)noiseHeight, dLinearDepth, (int)depthWidth, (int)depthHeight, (float4*)dClouds,
                  (int)width, (int)height, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_clouds");
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_sun_clouds(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params, const float* dClouds, int32_t cloudsWidth,
                              int32_t cloudsHeight, float* dSun, int32_t width, int32_t height)
{
    if (!ctx || !frame || !params || !aligned(dSun, 16) || !aligned(dClouds, 16) || !extent_ok(width, height) || !extent_ok(cloudsWidth, cloudsHeight) ||
        (const void*)dSun == dClouds)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SkyUniforms U;
    if (!sky_uniforms(frame->view, frame->invProjection, frame->cameraPosition, params, &U)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    Mat4 projView;
    if (sailor_host_mat4_mul(frame->projection, frame->view, projView.m) != SAILOR_HIP_OK) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_sun_clouds, texel_grid(width, height), dim3(256), (const float4*)dClouds, (int)cloudsWidth, (int)cloudsHeight, (float4*)dSun,
                  (int)width, (int)height, U, projView);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_sun_clouds");
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_blit_clouds(SailorHipContext* ctx, const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight, float* dTarget, int32_t width,
                               int32_t height, const SailorBand* band)
{
    if (!ctx || !band || !extent_ok(width, height) || !extent_ok(cloudsWidth, cloudsHeight)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!sailor_hip_band_is_valid(width, height, band)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!aligned(dClouds, 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!band->fbRowCount) return SAILOR_HIP_OK; // a rank without rows holds no target
    if (!aligned(dTarget, 16) || (const void*)dTarget == dClouds) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_blit_clouds, texel_grid(width, band->fbRowCount), dim3(256), (const float4*)dClouds, (int)cloudsWidth, (int)cloudsHeight,
                  (float4*)dTarget, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_blit_clouds");
    return SAILOR_HIP_OK;
}

} // extern "C"
