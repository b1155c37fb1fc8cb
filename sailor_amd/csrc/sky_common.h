// What sky.hip (FILL, ENV, SUN, COMPOSE) and sky_clouds.hip (CLOUDS, SUN behind clouds, the clouds blit) share: the constants of Sky.shader, the fp32 vector
// vocabulary in the library's conventions (sky.hip's header lists them), RaySphereIntersect, IntersectSphere, the per-draw uniforms and the texel of the
// SUN define set.  Moved here unchanged from sky.hip; every function is inlined into its kernel.
#pragma once
#include "common.h"
#include "sampling.h"
#include "texel_pass.h"
#include "canonical_math.h"
#include <math.h>

#define SKY_R 6371000.0f          // Sky.shader:161
#define SKY_OUTER_R 6531000.0f    // R + AtmosphereR (:162), exact in fp32
#define SKY_MAX_CAST 1600000.0f   // AtmosphereR * 10 (:230)
#define SKY_SUN_R 0.0095120445f   // radians(0.545) (:166)
#define SKY_ZETA 0.99995476f      // cos(SunAngularR) (:311)
#define SKY_H0R 7994.0f
#define SKY_H0MIE 1200.0f
#define SKY_LOG2E 1.442695f
#define SKY_PI 3.14159265359f     // Math.glsl:1
#define SKY_STEPS 127             // INTEGRAL_STEPS_2 - 1 (:318)

struct S3 { float x, y, z; };

__host__ __device__ __forceinline__ float sky_dot(S3 a, S3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ __forceinline__ float sky_len(S3 a) { return sqrtf(sky_dot(a, a)); }
__host__ __device__ __forceinline__ S3 sky_sub(S3 a, S3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ S3 sky_madd(S3 a, S3 d, float t) { return {a.x + d.x * t, a.y + d.y * t, a.z + d.z * t}; }
__host__ __device__ __forceinline__ S3 sky_normalize(S3 a) { const float l = sky_len(a); return {a.x / l, a.y / l, a.z / l}; }
__host__ __device__ __forceinline__ S3 sky_cross(S3 a, S3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
__device__ __forceinline__ float sky_exp(float x) { return canonical_exp2f(x * SKY_LOG2E); }

// Math.glsl:242-264 with s0 = 0, a = 1
__device__ __forceinline__ float2 ray_sphere(S3 r0, S3 rd, float sr)
{
    const float b = 2.0f * sky_dot(rd, r0);
    const float c = sky_dot(r0, r0) - sr * sr;
    const float disc = b * b - 4.0f * c;
    if (disc < 0.0f) return make_float2(-1.0f, -1.0f);
    const float tmp = sqrtf(disc);
    const float x1 = (-b + tmp) / 2.0f, x2 = (-b - tmp) / 2.0f;
    return x1 < x2 ? make_float2(x1, x2) : make_float2(x2, x1);
}

// Sky.shader:218-245; EARTH = the FILL define
template <bool EARTH>
__device__ __forceinline__ S3 intersect_sphere(S3 origin, S3 direction)
{
    const float2 i = ray_sphere(origin, direction, SKY_OUTER_R);
    const float outer = i.x < 0.0f ? i.y : i.x;
    if (outer <= 0.0f) return origin;
    float shift = outer < SKY_MAX_CAST ? outer : SKY_MAX_CAST;
    if (EARTH) {
        const float2 t = ray_sphere(origin, direction, SKY_R);
        const float inner = t.x > 0.0f ? t.x : t.y;
        if (inner > 0.0f) shift = inner * 3.0f;
    }
    return sky_madd(origin, direction, shift);
}

struct SkyUniforms {
    Mat4 invProjection, invView;
    S3 origin;   // vec3(0, R, 0) + cameraPosition.xyz * 0.01 (:610)
    S3 sun;      // dirToSun = normalize(-data.lightDirection.xyz) (:611)
    S3 right;    // normalize(cross(dirToSun, vec3(0, 1, 0))) (:623, :699)
    S3 up;       // cross(right, dirToSun)
    S3 axis2;    // cross(dirToSun, up) (:703)
};

// :729-731 (FILL, ENV) and :617-619 (COMPOSE): the world-space view direction of texture coordinate (tx, ty)
__device__ __forceinline__ S3 sky_view_direction(const SkyUniforms& U, float tx, float ty)
{
    const float4 v = glsl_mul(U.invProjection, tx * 2.0f - 1.0f, ty * 2.0f - 1.0f, 1.0f, 1.0f);
    // ClipSpaceToViewSpace negates z, main() negates it again: both exact
    const float4 w = glsl_mul(U.invView, v.x / v.w, v.y / v.w, v.z / v.w, 0.0f);
    const float l = sqrtf(((w.x * w.x + w.y * w.y) + w.z * w.z) + w.w * w.w);
    return {w.x / l, w.y / l, w.z / l};
}

struct Q4 { float x, y, z, w; };
__device__ __forceinline__ Q4 quat_mult(Q4 a, Q4 b) // Math.glsl:47-55
{
    Q4 r;
    r.x = (((a.w * b.x) + (a.x * b.w)) + (a.y * b.z)) - (a.z * b.y);
    r.y = (((a.w * b.y) - (a.x * b.z)) + (a.y * b.w)) + (a.z * b.x);
    r.z = (((a.w * b.z) + (a.x * b.y)) - (a.y * b.x)) + (a.z * b.w);
    r.w = (((a.w * b.w) - (a.x * b.x)) - (a.y * b.y)) - (a.z * b.z);
    return r;
}
__device__ __forceinline__ S3 sky_rotate(S3 v, S3 axis, float angleRad) // Math.glsl:30-40, :57-74
{
    const float half = angleRad / 2.0f, x2 = half * half;
    const float s = half * (1.0f + x2 * (-0.16666667f + x2 * 0.008333334f));
    const float c = 1.0f + x2 * (-0.5f + x2 * 0.041666668f);
    const Q4 q = {axis.x * s, axis.y * s, axis.z * s, c};
    const Q4 conj = {-q.x, -q.y, -q.z, q.w};
    const Q4 r = quat_mult(quat_mult(q, {v.x, v.y, v.z, 0.0f}), conj);
    return {r.x, r.y, r.z};
}

// SUN (:693-715 and the SUN branches of SkyLighting) for texture coordinate (tx, ty), once the clouds test (:710-712) has let the texel through:
// the value of all three colour channels, 0 where SkyLighting returns early
__device__ __forceinline__ float sky_sun_texel(const SkyUniforms& U, float tx, float ty)
{
    const float ax = -SKY_SUN_R * (1.0f - tx) + SKY_SUN_R * tx, ay = -SKY_SUN_R * (1.0f - ty) + SKY_SUN_R * ty; // :696-697
    const S3 viewDir = sky_rotate(U.sun, U.up, ax);                           // :702
    const S3 direction = sky_normalize(sky_rotate(viewDir, U.axis2, ay));     // :703
    const S3 destination = intersect_sphere<false>(U.origin, direction);
    if (sky_len(sky_sub(destination, U.origin)) < 0.01f) return 0.0f;              // :281-284
    const float theta = sky_dot(direction, U.sun);
    if (theta < SKY_ZETA) return 0.0f;                                             // :310-315
    const float2 e = ray_sphere(U.origin, direction, SKY_R);                  // :362
    if (!((e.x < e.y ? e.y : e.x) < 0.0f)) return 0.0f;                            // :363, :371-374
    const float q = (1.0f - theta) / (1.0f - SKY_ZETA);
    const float t = 1.0f - q * q;                                             // :365
    const float attenuation = 0.83f * (1.0f - t) + 1.0f * t;                  // :366
    const float v = (attenuation * 1.0f) * 12000000.0f;                       // :367
    return v;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
static bool sky_uniforms(const float* view16, const float* invProjection16, const float* cameraPosition3, const SailorSkyParams* p, SkyUniforms* U)
{
    memcpy(U->invProjection.m, invProjection16, sizeof U->invProjection.m);
    if (sailor_host_mat4_inverse(view16, U->invView.m) != SAILOR_HIP_OK) return false;
    U->origin = {0.0f + cameraPosition3[0] * 0.01f, SKY_R + cameraPosition3[1] * 0.01f, 0.0f + cameraPosition3[2] * 0.01f};
    U->sun = sky_normalize({-p->lightDirection[0], -p->lightDirection[1], -p->lightDirection[2]});
    U->right = sky_normalize(sky_cross(U->sun, {0.0f, 1.0f, 0.0f}));
    U->up = sky_cross(U->right, U->sun);
    U->axis2 = sky_cross(U->sun, U->up);
    return true;
}
