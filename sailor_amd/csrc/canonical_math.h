// The two transcendental functions of the post-processing nodes (EyeAdaptation's log2 / exp2, the HBAO blur's exp2) as fixed fp32 algorithms
// (Cephes' single-precision forms), not v_log_f32 / v_exp_f32: tests/eye_adaptation_ref.py and tests/hbao_ref.py restate them and reproduce the
// kernels' results bit for bit.
#pragma once
#include "common.h"
#include <math.h>

// log2 of a finite x >= 2^-126 (the histogram only asks for lum >= 0.005): mantissa in [sqrt(1/2), sqrt(2)), degree-8 polynomial
__host__ __device__ __forceinline__ float canonical_log2f(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    int e = (int)(u >> 23) - 126;
    u = (u & 0x007fffffu) | 0x3f000000u;
    float m;
    memcpy(&m, &u, 4); // [0.5, 1)
    if (m < 0.707106781186547524f) { e -= 1; m = (m + m) - 1.0f; }
    else m = m - 1.0f;
    const float z = m * m;
    float p = 7.0376836292e-2f;
    p = p * m + -1.1514610310e-1f;
    p = p * m + 1.1676998740e-1f;
    p = p * m + -1.2420140846e-1f;
    p = p * m + 1.4249322787e-1f;
    p = p * m + -1.6668057665e-1f;
    p = p * m + 2.0000714765e-1f;
    p = p * m + -2.4999993993e-1f;
    p = p * m + 3.3333331174e-1f;
    float y = m * (z * p);
    y = y - 0.5f * z;
    float r = y * 0.44269504088896340736f;
    r = r + m * 0.44269504088896340736f;
    r = r + y;
    r = r + m;
    return r + (float)e;
}

// exp2 with the argument clamped to [-126, 127]; NaN in, NaN out
__host__ __device__ __forceinline__ float canonical_exp2f(float x)
{
    if (x > 127.0f) x = 127.0f;
    if (x < -126.0f) x = -126.0f;
    float n = floorf(x);
    float r = x - n;
    if (r > 0.5f) { n = n + 1.0f; r = r - 1.0f; }
    float p = 1.535336188319500e-4f;
    p = p * r + 1.339887440266574e-3f;
    p = p * r + 9.618437357674640e-3f;
    p = p * r + 5.550332471162809e-2f;
    p = p * r + 2.402264791363012e-1f;
    p = p * r + 6.931472028550421e-1f;
    const float y = p * r + 1.0f;
    return x != x ? x : ldexpf(y, (int)n);
}
