// The end of the Sky node for gfx950: the star points and the sun-shaft pass, the first and the last draw of the region "Stars & Clouds".
//
// Replaces the two draws of SkyNode::Process (FrameGraph/SkyNode.cpp:692-747) that sky_clouds.hip left out; the clouds blit between them is there:
//   Stars.shader      -> k_sky_stars_project, k_sky_stars_blend   the point list under EBlendMode::Additive   (SkyNode.cpp:694-720, Stars.shader:49-59, :101-128,
//                                                                  material :517-522)
//   SunShafts.shader  -> k_sky_sun_shafts                         the quad under EBlendMode::Multiply         (SkyNode.cpp:733-739, SunShafts.shader:96-140,
//                                                                  material :453-454)
// Images are RGBA32F in device memory, 16-byte aligned, row 0 = top; texel (i, j) of a w x h target has the quad's inTexcoord ((i + 0.5) / w, (j + 0.5) / h).
// tests/stars_ref.py (Ref32) restates this file operation by operation in NumPy float32 and is its specification; the conventions are those sky.hip's
// header lists (no contraction, dot = (x x + y y) + z z, mat4 * vec4 row by row left to right, IEEE division and square root, min, max and clamp(x, 0, 1)
// by their GLSL definitions (common.h), mix(a, b, t) = a (1 - t) + b t, pow(x, 3) = (x * x) * x).  Both draws work in place on the rows of `band` of the
// target, like the clouds blit.  Everything records only: no allocation, no synchronisation, capturable; a refused call records nothing.
//
// Decisions, SunShafts.shader (line numbers of that file)
//   Vertex shader
//   * it does not flip (:22): fragTexcoord = inTexcoord.
//   Uniform quantities, computed once on the host in fp32
//   * dirToSun = normalize(-lightDirection.xyz) (:101) as sky_uniforms computes it for every other draw of the node.
//   * uvView = ((projection * view) * vec4(dirToSun, 0) + 1) * 0.5, then all of it divided by its own w (:103-104): projection * view by
//     sailor_host_mat4_mul, the matrix * vector product row by row left to right, x / w and y / w.
//   * the two early-outs -- sunShaftsIntensity == 0 (:108) and uvView outside [-0.51, 1.51] (:120-124, 1 + border in fp32) -- do not vary per fragment.
//     A fragment that returns early still writes (0, 0, 0, 0) and that value is still blended: the pass is recorded in every case.  A NaN uvView fails
//     every comparison and falls through to the loop, as written.
//   * texelSize = 1.0f / textureSize (:113), fade (:118: max(0, max(uvView.x - 1, uvView.y - 1))), mix(0, 1.0f, 1 - fade / border) (:138) taken by its
//     definition 0 * (1 - t) + 1 * t, and clamp(1 - outColor.r, 0, 1) with r = 0.005 (:137 comes before :138).
//   The tap loop (:126-132)
//   * texture(cloudsSampler, uv) is accumulated in loop order, unreassociated, uv += blurDirection follows each tap, and the sum is divided by
//     float(sunShaftsDistance).  blurDirection = ((uvView.xy - fragTexcoord) * texelSize) * blurRadius, left to right.
//   * the sampler is the clouds' colorSampler of sampling.h: bilinear, clamp-to-edge, the base level only.  Every tap index is clamped after the
//     saturating conversion: no uv, however far the walk carries it or whatever a NaN uvView makes of it, fetches outside the plane.
//   * sunShaftsDistance outside 1 .. 1024 is refused with the invalid-argument status: the editor's slider is 1 .. 100, and an unbounded count would be
//     an unbounded kernel.
//   The tail (:134-139), operation by operation, left to right
//   * a = 1 - clamp(1 - sum.a * sunShaftsIntensity, 0, 1);  rgb = 0.005;  outColor = ((a * outColor) * mixTerm) * clampTerm, so rgb = ((a * 0.005) *
//     mixTerm) * clampTerm and alpha = ((a * a) * mixTerm) * clampTerm;  alpha *= clamp(pow(g, 3), 0, 1) with g from a second fetch at fragTexcoord.
//   BLEND STATE EBlendMode::Multiply (VulkanPipileneStates.cpp:248-254) -- a named decision
//   * the state sets VK_BLEND_OP_MULTIPLY_EXT for colour and SUBTRACT with SRC_ALPHA / DST_ALPHA for alpha.  That is not valid Vulkan (an advanced blend
//     op must be the same for colour and alpha) and no hardware can be asked.  This tree's reading:
//         rgb = Cs * Cd + Cs * (1 - Ad) + Cd * (1 - As), summed left to right;      a = As * As - Ad * Ad.
//     The colour line is VK_EXT_blend_operation_advanced's MULTIPLY equation for premultiplied operands and uncorrelated overlap with the quotients
//     cancelled; the alpha line is the state as written, the way the clouds blit restates its own.  The extension's "the quotient is 0 where alpha is 0"
//     rule is NOT restated: this tree stores the target's alpha as 0 where the reference leaves it undefined, and that rule would black out the sky.
//
// Decisions, Stars.shader
//   Vertex shader (:49-59)
//   * gl_Position = ((projection * view) * model) * vec4(p, 1): the matrix products once on the host (sailor_host_mat4_mul, twice), the matrix * vector
//     product per star.  gl_PointSize = 1, no depth test (material :520: depth test and write off).
//   * a star is dropped if a clip coordinate is not finite, if w <= 0, or if it lies outside -w <= x, y <= w or 0 <= z <= w (the clip volume of a point).
//   * the viewport is the frame's (VulkanDevice.cpp:681-685: y = H, height -H): xf = ((ndc.x + 1) * 0.5) * W, yf = H - ((ndc.y + 1) * 0.5) * H.  The one
//     fragment is pixel (floor(xf), floor(yf)); it is dropped if it lies outside the target or outside `band`.  A point exactly on a pixel edge goes
//     right / down: that is a decision.  frame->viewportSize must equal (width, height).
//   * fragUV.xy = (ndc.xy + 1) * 0.5; fragWPosition is never written, and never read.
//   Fragment shader (:101-128), as written
//   * origin = vec3(0, R + 1000, 0) + cameraPosition.xyz: there is no 0.01 factor here, unlike Sky.shader:610.
//   * viewportPos = gl_FragCoord.xy / viewportSize with y then 1 - y, from the pixel centre; the view ray through ScreenSpaceToViewSpace and
//     inverse(view) as COMPOSE builds it (sky_view_direction); RaySphereIntersect of Math.glsl (ray_sphere).
//   * clouds = the alpha of a bilinear clamp-to-edge fetch at viewportPos.  A NULL plane is the cleared m_pCloudsTexture, as in sailor_hip_sky_sun.
//   * mask = clamp(1 - 1000 * clamp(length(viewportPos - fragUV), 0, 1), 0, 1);  outColor = mask * fragColor;  a = clamp(1, 0, 1) = 1;
//     rgb *= (a * (1 - clouds)) * 0.15, the right-hand side first.
//   * a fragment whose ray hits the Earth is (0, 0, 0, 0) and is STILL ADDED: -0 + 0 = +0 is a visible bit.
//   Additive blend and order
//   * rgb and a are added to the target.  Stars on one pixel blend in index order, Vulkan's primitive order, and the result is that sequential sum bit
//     for bit on every run: no float atomics.  k_sky_stars_project writes each star's pixel (or -1) and fragment into a workspace; in
//     k_sky_stars_blend the first star of a pixel adds itself and then the later stars of that pixel, in order, and stores once.  The scan is
//     count^2 / 2 four-byte loads that a wave shares; count above 65 536 is refused (the catalogue has 9 110).
//   * the workspace (sailor_hip_sky_stars_workspace_bytes) is the caller's, bound to the context beforehand; it is never allocated inside the call.
//
// Shape, one line per kernel (tests/test_stars_resources_cpu.py reads the occupancy figures).  No LDS, no scratch, no spills.
//   k_sky_sun_shafts: 8 waves per SIMD -- a texel per lane, texel_grid blocks; per tap four float4 loads of a plane that stays in L2
//   k_sky_stars_project: 8 waves per SIMD -- a star per lane, 256 per block
//   k_sky_stars_blend: 8 waves per SIMD -- a star per lane, 256 per block; the scan's loads are the same address in every lane of a wave
#include "sky_common.h"

#define SHAFTS_MAX_DISTANCE 1024   // sunShaftsDistance, refused above
#define STARS_MAX_COUNT 65536
#define STARS_ORIGIN_R 6372000.0f  // R + 1000 (Stars.shader:103), exact in fp32

struct ShaftUniforms {
    float uvx, uvy;       // uvView.xy (:103-104)
    float tsx, tsy;       // texelSize (:113)
    float intensity;      // sunShaftsIntensity
    float countF;         // float(sunShaftsDistance) (:98)
    float mixTerm;        // mix(0, 1.0f, 1 - fade / border) (:138)
    float clampTerm;      // clamp(1 - 0.005, 0, 1) (:137-138)
    int count;
    int early;            // :108-111, :120-124
};

// ---- a. Sun Shafts (SunShafts.shader:96-140 under EBlendMode::Multiply) ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sky_sun_shafts(const float4* __restrict__ clouds, int CW, int CH, float4* __restrict__ target, int W, int H,
                                                        int rowBegin, int rowCount, const ShaftUniforms U)
{
    const int i = texel_i(), r = texel_j();
    if (i >= W || r >= rowCount) return;
    const int j = rowBegin + r;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H; // fragTexcoord (:22)
    float4 src = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                               // :106
    if (!U.early) {
        const float bx = ((U.uvx - u) * U.tsx) * 5.0f, by = ((U.uvy - v) * U.tsy) * 5.0f; // :114
        float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float x = u, y = v;
#pragma unroll 1
        for (int k = 0; k < U.count; k++) { // :126-130
            const float4 t = sample_clamp_f4_saturating(clouds, CW, CH, x, y);
            sum.x = sum.x + t.x; sum.y = sum.y + t.y; sum.z = sum.z + t.z; sum.w = sum.w + t.w;
            x = x + bx; y = y + by;
        }
        const float avgA = sum.w / U.countF;                                  // :132 (rgb is overwritten at :137)
        const float a = 1.0f - glsl_saturate(1.0f - avgA * U.intensity);     // :134
        const float g = sample_clamp_f4_saturating(clouds, CW, CH, u, v).y;  // :139
        src.x = src.y = src.z = ((a * 0.005f) * U.mixTerm) * U.clampTerm;    // :137-138
        src.w = (((a * a) * U.mixTerm) * U.clampTerm) * glsl_saturate((g * g) * g);
    }
    float4* __restrict__ t = target + (size_t)r * (size_t)W + i;
    const float4 dst = *t;
    const float kd = 1.0f - dst.w, ks = 1.0f - src.w;
    *t = make_float4((src.x * dst.x + src.x * kd) + dst.x * ks, (src.y * dst.y + src.y * kd) + dst.y * ks, (src.z * dst.z + src.z * kd) + dst.z * ks,
                     src.w * src.w - dst.w * dst.w);
}

// ---- b. Stars (Stars.shader under EBlendMode::Additive, a point list) ------------------------------------------------------------------------------
struct StarsUniforms {
    Mat4 clipFromModel;   // (projection * view) * model (:52)
    SkyUniforms sky;      // invProjection, invView and origin = vec3(0, R + 1000, 0) + cameraPosition.xyz (:103); the sun's members are not set
};

__device__ __forceinline__ bool stars_finite(float x) { return fabsf(x) < __builtin_inff(); } // false for NaN

// vertex shader, rasteriser and fragment shader of one star: its pixel inside the band's rows (or -1) and its fragment
__global__ __launch_bounds__(256) void k_sky_stars_project(const float* __restrict__ positions, const float4* __restrict__ colors, int count,
                                                           const float4* __restrict__ clouds, int CW, int CH, float4* __restrict__ fragments,
                                                           int* __restrict__ pixels, int W, int H, int rowBegin, int rowCount, const StarsUniforms U)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= count) return;
    const float4 clip = glsl_mul(U.clipFromModel, positions[3 * (size_t)s], positions[3 * (size_t)s + 1], positions[3 * (size_t)s + 2], 1.0f); // :52
    int pixel = -1;
    float4 frag = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // :113
    const bool inside = stars_finite(clip.x) && stars_finite(clip.y) && stars_finite(clip.z) && stars_finite(clip.w) && clip.w > 0.0f && -clip.w <= clip.x &&
                        clip.x <= clip.w && -clip.w <= clip.y && clip.y <= clip.w && 0.0f <= clip.z && clip.z <= clip.w;
    if (inside) {
        const float nx = clip.x / clip.w, ny = clip.y / clip.w;                                      // :54
        const float fu = (nx + 1.0f) * 0.5f, fv = (ny + 1.0f) * 0.5f;                                // fragUV (:57)
        const float xf = fu * (float)W, yf = (float)H - fv * (float)H;                               // the viewport: y = H, height -H
        const float px = floorf(xf), py = floorf(yf);                                                // |ndc| <= 1: 0 <= xf <= W, 0 <= yf <= H
        const int ix = (int)px, iy = (int)py;
        if (ix >= 0 && ix < W && iy >= rowBegin && iy < rowBegin + rowCount) {
            pixel = (iy - rowBegin) * W + ix;
            const float vx = (px + 0.5f) / (float)W, vy = 1.0f - (py + 0.5f) / (float)H;             // viewportPos (:104-105)
            const S3 dir = sky_view_direction(U.sky, vx, vy);                                        // :107-111
            const float cloudsA = clouds ? sample_clamp_f4_saturating(clouds, CW, CH, vx, vy).w : 0.0f; // :115
            const float2 e = ray_sphere(U.sky.origin, dir, SKY_R);                                   // :117
            if (glsl_max(e.x, e.y) < 0.0f) {
                const float dx = vx - fu, dy = vy - fv;
                const float mask = glsl_saturate(1.0f - 1000.0f * glsl_saturate(sqrtf(dx * dx + dy * dy))); // :120
                const float4 c = colors[s];
                const float k = (1.0f * (1.0f - cloudsA)) * 0.15f;                                   // :124-126
                frag = make_float4((mask * c.x) * k, (mask * c.y) * k, (mask * c.z) * k, 1.0f);
            }
        }
    }
    pixels[s] = pixel;
    fragments[s] = frag;
}

// the additive blend in primitive order: the first star of a pixel adds itself and every later star of that pixel, in index order, and stores once
__global__ __launch_bounds__(256) void k_sky_stars_blend(const float4* __restrict__ fragments, const int* __restrict__ pixels, int count,
                                                         float4* __restrict__ target)
{
    const int s = (int)(blockIdx.x * 256 + threadIdx.x);
    if (s >= count) return;
    const int pixel = pixels[s];
    if (pixel < 0) return;
    for (int k = 0; k < s; k++)
        if (pixels[k] == pixel) return; // an earlier star owns the pixel
    float4 t = target[pixel];
    for (int k = s; k < count; k++) {
        if (pixels[k] != pixel) continue;
        const float4 f = fragments[k];
        t.x = t.x + f.x; t.y = t.y + f.y; t.z = t.z + f.z; t.w = t.w + f.w;
    }
    target[pixel] = t;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static void stars_host_mul(const float* m, float x, float y, float z, float w, float* out4) // glsl_mul (common.h) on the host
{
    for (int r = 0; r < 4; r++) out4[r] = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w;
}
static float stars_host_max(float x, float y) { return x < y ? y : x; }                      // glsl_max
static float stars_host_saturate(float x) { const float a = x < 0.0f ? 0.0f : x; return 1.0f < a ? 1.0f : a; } // glsl_saturate

static size_t stars_fragment_bytes(int32_t count) { return align_up((size_t)count * sizeof(float4), 16); }

extern "C" {

int sailor_hip_sky_sun_shafts(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorSkyParams* params, const float* dClouds,
                              int32_t cloudsWidth, int32_t cloudsHeight, float* dTarget, int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx || !frame || !params || !band || !extent_ok(width, height) || !extent_ok(cloudsWidth, cloudsHeight)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!sailor_hip_band_is_valid(width, height, band)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!aligned(dClouds, 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (params->sunShaftsDistance < 1 || params->sunShaftsDistance > SHAFTS_MAX_DISTANCE) {
        ctx->lastError = "sailor_hip_sky_sun_shafts: sunShaftsDistance outside 1 .. 1024";
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    }
    if (!band->fbRowCount) return SAILOR_HIP_OK; // a rank without rows holds no target
    if (!aligned(dTarget, 16) || overlaps(dTarget, (size_t)band->fbRowCount * (size_t)width * sizeof(float4), dClouds,
                                          (size_t)cloudsHeight * (size_t)cloudsWidth * sizeof(float4)))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SkyUniforms S;
    if (!sky_uniforms(frame->view, frame->invProjection, frame->cameraPosition, params, &S)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    float projView[16], clip[4];
    if (sailor_host_mat4_mul(frame->projection, frame->view, projView) != SAILOR_HIP_OK) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    stars_host_mul(projView, S.sun.x, S.sun.y, S.sun.z, 0.0f, clip); // :103
    ShaftUniforms U;
    const float w = (clip[3] + 1.0f) * 0.5f;
    U.uvx = ((clip[0] + 1.0f) * 0.5f) / w; // :104
    U.uvy = ((clip[1] + 1.0f) * 0.5f) / w;
    U.tsx = 1.0f / (float)cloudsWidth;     // :113
    U.tsy = 1.0f / (float)cloudsHeight;
    U.intensity = params->sunShaftsIntensity;
    U.count = params->sunShaftsDistance;
    U.countF = (float)params->sunShaftsDistance; // :98
    const float border = 0.51f;
    const float fade = stars_host_max(0.0f, stars_host_max(U.uvx - 1.0f, U.uvy - 1.0f)); // :118
    const float t = 1.0f - fade / border;
    U.mixTerm = 0.0f * (1.0f - t) + 1.0f * t;               // mix(0, 1.0f, t) (:138)
    U.clampTerm = stars_host_saturate(1.0f - 0.005f);       // :137-138
    U.early = (params->sunShaftsIntensity == 0.0f || U.uvx > 1.0f + border || U.uvy > 1.0f + border || U.uvx < -border || U.uvy < -border) ? 1 : 0;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_sun_shafts, texel_grid(width, band->fbRowCount), dim3(256), (const float4*)dClouds, (int)cloudsWidth, (int)cloudsHeight,
                  (float4*)dTarget, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_sun_shafts");
    return SAILOR_HIP_OK;
}

size_t sailor_hip_sky_stars_workspace_bytes(int32_t count)
{
    if (count < 0 || count > STARS_MAX_COUNT) return 0;
    return stars_fragment_bytes(count) + align_up((size_t)count * sizeof(int), 16);
}

int sailor_hip_sky_stars_bind_workspace(SailorHipContext* ctx, void* dWorkspace, size_t workspaceBytes)
{
    if (!ctx || (dWorkspace && !aligned(dWorkspace, 16)) || (!dWorkspace && workspaceBytes)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    ctx->starsWorkspace = dWorkspace;
    ctx->starsWorkspaceBytes = workspaceBytes;
    return SAILOR_HIP_OK;
}

int sailor_hip_sky_stars(SailorHipContext* ctx, const SailorUboFrameData* frame, const float* model16, const float* dPositions, const float* dColors,
                         int32_t count, const float* dClouds, int32_t cloudsWidth, int32_t cloudsHeight, float* dTarget, int32_t width, int32_t height,
                         const SailorBand* band)
{
    if (!ctx || !frame || !model16 || !band || !extent_ok(width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!sailor_hip_band_is_valid(width, height, band)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (count < 0 || count > STARS_MAX_COUNT) {
        ctx->lastError = "sailor_hip_sky_stars: count outside 0 .. 65536";
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    }
    if (frame->viewportSize[0] != width || frame->viewportSize[1] != height) {
        ctx->lastError = "sailor_hip_sky_stars: frame->viewportSize is not (width, height)";
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    }
    if (dClouds && (!aligned(dClouds, 16) || !extent_ok(cloudsWidth, cloudsHeight))) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (count && (!aligned(dPositions, 16) || !aligned(dColors, 16))) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!count || !band->fbRowCount) return SAILOR_HIP_OK; // no star, or a rank without rows: nothing to blend
    const size_t targetBytes = (size_t)band->fbRowCount * (size_t)width * sizeof(float4), need = sailor_hip_sky_stars_workspace_bytes(count);
    if (!aligned(dTarget, 16)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if ((dClouds && overlaps(dTarget, targetBytes, dClouds, (size_t)cloudsHeight * (size_t)cloudsWidth * sizeof(float4))) ||
        overlaps(dTarget, targetBytes, dPositions, (size_t)count * 12) || overlaps(dTarget, targetBytes, dColors, (size_t)count * 16))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!ctx->starsWorkspace || ctx->starsWorkspaceBytes < need || overlaps(dTarget, targetBytes, ctx->starsWorkspace, need)) {
        ctx->lastError = "sailor_hip_sky_stars: no workspace of sailor_hip_sky_stars_workspace_bytes(count) bound (sailor_hip_sky_stars_bind_workspace)";
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    }
    StarsUniforms U = {};
    float projView[16];
    if (sailor_host_mat4_mul(frame->projection, frame->view, projView) != SAILOR_HIP_OK ||
        sailor_host_mat4_mul(projView, model16, U.clipFromModel.m) != SAILOR_HIP_OK ||
        sailor_host_mat4_inverse(frame->view, U.sky.invView.m) != SAILOR_HIP_OK)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    memcpy(U.sky.invProjection.m, frame->invProjection, sizeof U.sky.invProjection.m);
    U.sky.origin = {0.0f + frame->cameraPosition[0], STARS_ORIGIN_R + frame->cameraPosition[1], 0.0f + frame->cameraPosition[2]};
    float4* fragments = (float4*)ctx->starsWorkspace;
    int* pixels = (int*)((char*)ctx->starsWorkspace + stars_fragment_bytes(count));
    const dim3 grid((unsigned)((count + 255) / 256));
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_sky_stars_project, grid, dim3(256), dPositions, (const float4*)dColors, (int)count, (const float4*)dClouds, (int)cloudsWidth,
                  (int)cloudsHeight, fragments, pixels, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, U);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_stars_project");
    sailor_launch(ctx, k_sky_stars_blend, grid, dim3(256), (const float4*)fragments, (const int*)pixels, (int)count, (float4*)dTarget);
    SAILOR_CHECK_LAUNCH(ctx, "k_sky_stars_blend");
    return SAILOR_HIP_OK;
}

} // extern "C"
