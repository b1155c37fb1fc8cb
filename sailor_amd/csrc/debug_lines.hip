// The DebugDraw node's pass: Gizmo.shader (:22 `gl_Position = viewProjection * vec4(inPosition, 1)`, :34 `outColor = fragColor`) under the material of
// RHI/DebugContext.cpp:272 -- LineList, lineWidth 1, depth test and write, GREATER_OR_EQUAL, blend None -- as a VISIBILITY-KEY line rasteriser for gfx950, in
// the style of surface.hip.  include/sailor_hip.h has the pinned rules; tests/lines_ref.py restates them sequentially and the kernels are held to it bit for bit.
//
//   (sailor_hip_surface_begin seeds one 64-bit key per pixel of the band from the current DepthBuffer: surface.hip)
//   k_debug_lines_draw     a lane per segment: vertex stage, the clip against five planes, the snap, the range of major-axis steps.  A segment of at most
//                          DBGL_LANE_FRAGMENTS steps is walked by its lane; a longer one is handed to the whole wave (ballot, the set-up record by __shfl), which
//                          produces its fragments 64 at a time.  Coverage is closed-form per step (no DDA), so any lane can produce any fragment; a fragment
//                          issues its key as the surface pass does (plain load, atomicMax only if larger).  A draw of few segments has few waves, so it is
//                          launched gridDim.y times over, as k_surface_visibility is: every slice sets all segments up again, slice 0 walks the short ones,
//                          and of a long segment's trips slice y takes those whose number is y modulo the slices.
//   k_debug_lines_resolve  a lane per pixel of the band: an owned pixel (low word != 0) -> the segment -> its set-up again -> t of this pixel -> the
//                          perspective-correct colour into the target (all four channels: blend None) and the key's depth into the depth attachment.
//
// Keys are order-free (the maximum does not depend on who issues a fragment or when), so the hand-over changes no bit.
#include "surface_common.h"

#define DBGL_VERTEX_FLOATS 7
#define DBGL_LANE_FRAGMENTS 64 // the major-axis steps a lane walks on its own
// 0 leaves every segment to its lane: for the measurement in DESIGN.md only, never shipped
#ifndef SAILOR_DEBUG_LINES_WAVE_HANDOVER
#define SAILOR_DEBUG_LINES_WAVE_HANDOVER 1
#endif

// a set-up segment: the snapped end points (1/256 pixel; |.| < 1e9, so they fit), their depth, and the closed range [m0, m0 + n) of major-axis pixel
// coordinates that can hold a fragment, already cut to the frame (x-major) or to the band's rows (y-major).  n == 0: nothing to draw.
struct DbgLine { int X0, Y0, X1, Y1; float z0, z1; int m0, n; bool xMajor; };
// what the colour of a fragment needs on top: clip w and colour of the two clipped end points
struct DbgLineColor { float w0, w1, c0[4], c1[4]; };

__device__ __forceinline__ long long dbgl_floor_div(long long a, long long b) // b > 0
{
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// vertex stage, clip, snap, range.  C is filled only when wantColor (dead code in the draw kernel).
__device__ __forceinline__ DbgLine dbgl_setup(const Mat4& VP, const float* __restrict__ vertices, const uint32_t* __restrict__ indices, uint32_t segment, int W, int H,
                                              int rowBegin, int rowEnd, bool wantColor, DbgLineColor& C)
{
    DbgLine L;
    L.X0 = L.Y0 = L.X1 = L.Y1 = 0; L.z0 = L.z1 = 0.0f; L.m0 = 0; L.n = 0; L.xMajor = true;
    const uint32_t ia = indices ? indices[2 * (size_t)segment] : 2u * segment, ib = indices ? indices[2 * (size_t)segment + 1] : 2u * segment + 1u;
    const float* __restrict__ pa = vertices + DBGL_VERTEX_FLOATS * (size_t)ia;
    const float* __restrict__ pb = vertices + DBGL_VERTEX_FLOATS * (size_t)ib;
    const float4 A = glsl_mul(VP, pa[0], pa[1], pa[2], 1.0f), B = glsl_mul(VP, pb[0], pb[1], pb[2], 1.0f);
    // the view volume's near and side planes (the far plane is the per-fragment z > 0)
    float tIn = 0.0f, tOut = 1.0f;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const float dA = k == 0 ? A.w - A.z : (k == 1 ? A.w + A.x : (k == 2 ? A.w - A.x : (k == 3 ? A.w + A.y : A.w - A.y)));
        const float dB = k == 0 ? B.w - B.z : (k == 1 ? B.w + B.x : (k == 2 ? B.w - B.x : (k == 3 ? B.w + B.y : B.w - B.y)));
        if (dA < 0.0f && dB < 0.0f) return L;
        if (dA < 0.0f) { const float t = dA / (dA - dB); if (t > tIn) tIn = t; }
        else if (dB < 0.0f) { const float t = dA / (dA - dB); if (t < tOut) tOut = t; }
    }
    if (tIn > tOut) return L;
    // both clipped end points from the ORIGINAL ones; an end the planes did not move is the original, bit for bit
    float4 P0 = A, P1 = B;
    if (tIn > 0.0f) P0 = make_float4(A.x + (B.x - A.x) * tIn, A.y + (B.y - A.y) * tIn, A.z + (B.z - A.z) * tIn, A.w + (B.w - A.w) * tIn);
    if (tOut < 1.0f) P1 = make_float4(A.x + (B.x - A.x) * tOut, A.y + (B.y - A.y) * tOut, A.z + (B.z - A.z) * tOut, A.w + (B.w - A.w) * tOut);
    if (!(P0.w > 0.0f) || !(P1.w > 0.0f)) return L;
    long long X[2], Y[2];
    float Z[2];
#pragma unroll
    for (int k = 0; k < 2; k++) { // surface_setup's snap
        const float4 clip = k == 0 ? P0 : P1;
        const float nx = clip.x / clip.w, ny = clip.y / clip.w, nz = clip.z / clip.w;
        const float xf = (nx + 1.0f) * ((float)W * 0.5f);
        const float yf = (ny + 1.0f) * ((float)H * -0.5f) + (float)H;
        const float sx = xf * 256.0f, sy = yf * 256.0f;
        if (!(fabsf(sx) < 1.0e9f) || !(fabsf(sy) < 1.0e9f)) return L;
        X[k] = (long long)rintf(sx); Y[k] = (long long)rintf(sy); Z[k] = nz;
    }
    if (wantColor) {
        C.w0 = P0.w; C.w1 = P1.w;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float ca = pa[3 + c], cb = pb[3 + c];
            C.c0[c] = tIn > 0.0f ? ca + (cb - ca) * tIn : ca;
            C.c1[c] = tOut < 1.0f ? ca + (cb - ca) * tOut : cb;
        }
    }
    const long long dX = X[1] - X[0], dY = Y[1] - Y[0];
    if (dX == 0 && dY == 0) return L;
    const bool xMajor = (dX < 0 ? -dX : dX) >= (dY < 0 ? -dY : dY);
    const long long S0 = xMajor ? X[0] : Y[0], S1 = xMajor ? X[1] : Y[1];
    // pixel centres M = 256 m + 128 with S0 <= M < S1 (rising) or S1 < M <= S0 (falling): the start is included, the end is not
    long long lo, hi; // inclusive
    if (S1 > S0) { lo = surf_floor_div256(S0 - 128 + 255); hi = surf_floor_div256(S1 - 128 + 255) - 1; }
    else { lo = surf_floor_div256(S1 - 128) + 1; hi = surf_floor_div256(S0 - 128); }
    const long long first = xMajor ? 0 : rowBegin, last = xMajor ? W - 1 : rowEnd - 1;
    if (lo < first) lo = first;
    if (hi > last) hi = last;
    if (hi < lo) return L;
    L.X0 = (int)X[0]; L.Y0 = (int)Y[0]; L.X1 = (int)X[1]; L.Y1 = (int)Y[1];
    L.z0 = Z[0]; L.z1 = Z[1];
    L.m0 = (int)lo; L.n = (int)(hi - lo + 1); L.xMajor = xMajor;
    return L;
}

// the fragment of major-axis pixel coordinate m: its minor coordinate (the pixel that contains the line's point at that centre, an exact integer floor) and
// its parameter t.  false: the pixel is outside the frame or the band's rows.
__device__ __forceinline__ bool dbgl_fragment(const DbgLine& L, int m, int W, int rowBegin, int rowEnd, int& i, int& j, float& t)
{
    const long long S0 = L.xMajor ? L.X0 : L.Y0, T0 = L.xMajor ? L.Y0 : L.X0;
    const long long dS = L.xMajor ? (long long)L.X1 - L.X0 : (long long)L.Y1 - L.Y0, dT = L.xMajor ? (long long)L.Y1 - L.Y0 : (long long)L.X1 - L.X0;
    const long long M = 256ll * m + 128;
    long long num = T0 * dS + dT * (M - S0), den = 256ll * dS;
    if (den < 0) { num = -num; den = -den; }
    const long long minor = dbgl_floor_div(num, den);
    t = (float)(M - S0) / (float)dS;
    if (L.xMajor) { if (minor < rowBegin || minor >= rowEnd) return false; i = m; j = (int)minor; }
    else { if (minor < 0 || minor >= W) return false; i = (int)minor; j = m; }
    return true;
}

__device__ __forceinline__ void dbgl_issue(const DbgLine& L, int m, int W, int rowBegin, int rowEnd, unsigned long long* keys, unsigned int orderPlus1)
{
    int i, j;
    float t;
    if (!dbgl_fragment(L, m, W, rowBegin, rowEnd, i, j, t)) return;
    const float z = L.z0 + (L.z1 - L.z0) * t;
    if (z > 0.0f && z <= 1.0f) surf_fragment(keys + (size_t)(j - rowBegin) * W + i, z, orderPlus1);
}

__global__ __launch_bounds__(256) void k_debug_lines_draw(Mat4 VP, SailorDebugLinesDraw draw, int W, int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    const SurfWorkspace ws = surf_workspace(workspace, (size_t)rows * W);
    unsigned long long* keys = ws.keys;
    const unsigned long long id = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int rowEnd = rowBegin + rows;
    const int slice = (int)blockIdx.y, slices = (int)gridDim.y;
    DbgLine L;
    L.n = 0;
    if (id < draw.numSegments) {
        DbgLineColor unused;
        L = dbgl_setup(VP, reinterpret_cast<const float*>(draw.dVertices), draw.dIndices, (uint32_t)id, W, H, rowBegin, rowEnd, false, unused);
    }
    const unsigned int orderPlus1 = draw.primBase + (unsigned int)id + 1u; // (the entry point has checked the range)
#if SAILOR_DEBUG_LINES_WAVE_HANDOVER
    const bool own = L.n <= DBGL_LANE_FRAGMENTS;
#else
    const bool own = true;
#endif
    if (own && slice == 0) for (int k = 0; k < L.n; k++) dbgl_issue(L, L.m0 + k, W, rowBegin, rowEnd, keys, orderPlus1);
#if SAILOR_DEBUG_LINES_WAVE_HANDOVER
    // the long ones: the whole wave on one segment at a time, 64 fragments a trip
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(!own);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        DbgLine b;
        b.X0 = __shfl(L.X0, src, 64); b.Y0 = __shfl(L.Y0, src, 64); b.X1 = __shfl(L.X1, src, 64); b.Y1 = __shfl(L.Y1, src, 64);
        b.z0 = __shfl(L.z0, src, 64); b.z1 = __shfl(L.z1, src, 64);
        b.m0 = __shfl(L.m0, src, 64); b.n = __shfl(L.n, src, 64); b.xMajor = __shfl((int)L.xMajor, src, 64) != 0;
        const unsigned int bOrder = (unsigned int)__shfl((int)orderPlus1, src, 64);
        for (int k = 64 * slice + lane; k < b.n; k += 64 * slices) dbgl_issue(b, b.m0 + k, W, rowBegin, rowEnd, keys, bOrder);
    }
#endif
}

__global__ __launch_bounds__(256) void k_debug_lines_resolve(Mat4 VP, SailorDebugLinesDraw draw, int W, int H, int rowBegin, int rows, const void* __restrict__ workspace,
                                                             float4* __restrict__ target, float* __restrict__ depth)
{
    const int i = texel_i(), jb = texel_j();
    if (i >= W || jb >= rows) return;
    const SurfWorkspace ws = surf_workspace(const_cast<void*>(workspace), (size_t)rows * W);
    const size_t at = (size_t)jb * W + i;
    const unsigned long long key = ws.keys[at];
    const unsigned int low = (unsigned int)key;
    if (low == 0u) return; // no segment owns the pixel: colour and depth stay
    const unsigned int segment = (low - 1u) - draw.primBase;
    if (segment >= draw.numSegments) return; // (a key of another draw: not this pass's)
    DbgLineColor C;
    const DbgLine L = dbgl_setup(VP, reinterpret_cast<const float*>(draw.dVertices), draw.dIndices, segment, W, H, rowBegin, rowBegin + rows, true, C);
    if (L.n == 0) return;
    const int j = jb + rowBegin;
    const long long S0 = L.xMajor ? L.X0 : L.Y0, dS = L.xMajor ? (long long)L.X1 - L.X0 : (long long)L.Y1 - L.Y0;
    const long long M = 256ll * (L.xMajor ? i : j) + 128;
    const float t = (float)(M - S0) / (float)dS;
    const float q0 = (1.0f - t) / C.w0, q1 = t / C.w1;
    const float b = q1 / (q0 + q1);
    target[at] = make_float4(C.c0[0] + (C.c1[0] - C.c0[0]) * b, C.c0[1] + (C.c1[1] - C.c0[1]) * b, C.c0[2] + (C.c1[2] - C.c0[2]) * b, C.c0[3] + (C.c1[3] - C.c0[3]) * b);
    depth[(size_t)j * W + i] = __uint_as_float((unsigned int)(key >> 32));
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
static const char* dbgl_check(const float* viewProjection, const SailorDebugLinesDraw* draw, int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace,
                              size_t workspaceBytes)
{
    if (!viewProjection || !draw) return "the matrix or the draw is NULL";
    if (const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true)) return why;
    if (draw->numSegments && !aligned(draw->dVertices, 4)) return "the vertex buffer is NULL or not 4-byte aligned";
    if (draw->dIndices && !aligned(draw->dIndices, 4)) return "the index buffer is not 4-byte aligned";
    if ((unsigned long long)draw->primBase + draw->numSegments >= 0xFFFFFFFFull) return "primBase + the draw's segments reaches 2^32 - 1";
    return nullptr;
}

extern "C" {

int sailor_hip_debug_lines_prims(uint32_t numSegments, uint64_t* out)
{
    if (!out) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    *out = numSegments;
    return SAILOR_HIP_OK;
}

int sailor_hip_debug_lines_draw(SailorHipContext* ctx, const float* viewProjection, const SailorDebugLinesDraw* draw, int32_t width, int32_t height, const SailorBand* band,
                                void* dWorkspace, size_t workspaceBytes)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (const char* why = dbgl_check(viewProjection, draw, width, height, band, dWorkspace, workspaceBytes))
        return surf_refuse(ctx, "sailor_hip_debug_lines_draw", why);
    if (draw->numSegments == 0) return SAILOR_HIP_OK; // nothing to record
    Mat4 VP;
    memcpy(VP.m, viewProjection, 64);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_debug_lines_draw, dim3((unsigned)(((unsigned long long)draw->numSegments + 255) / 256), surf_slices(draw->numSegments)), dim3(256), VP, *draw,
                  (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
    SAILOR_CHECK_LAUNCH(ctx, "k_debug_lines_draw");
    return SAILOR_HIP_OK;
}

int sailor_hip_debug_lines_resolve(SailorHipContext* ctx, const float* viewProjection, const SailorDebugLinesDraw* draw, int32_t width, int32_t height, const SailorBand* band,
                                   const void* dWorkspace, size_t workspaceBytes, float* dTarget, float* dDepth)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = dbgl_check(viewProjection, draw, width, height, band, dWorkspace, workspaceBytes);
    if (!why && !aligned(dTarget, 16)) why = "the target is NULL or not 16-byte aligned";
    if (!why && !aligned(dDepth, 4)) why = "the depth attachment is NULL or not 4-byte aligned";
    if (why) return surf_refuse(ctx, "sailor_hip_debug_lines_resolve", why);
    if (draw->numSegments == 0) return SAILOR_HIP_OK;
    Mat4 VP;
    memcpy(VP.m, viewProjection, 64);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_debug_lines_resolve, texel_grid(width, band->fbRowCount), dim3(256), VP, *draw, (int)width, (int)height, (int)band->fbRowBegin,
                  (int)band->fbRowCount, dWorkspace, reinterpret_cast<float4*>(dTarget), dDepth);
    SAILOR_CHECK_LAUNCH(ctx, "k_debug_lines_resolve");
    return SAILOR_HIP_OK;
}

} // extern "C"
