// What the surface-pass translation units share (surface.hip: the Opaque queue; surface_masked.hip: the Masked queue with ALPHA_CUTOUT; surface_gltf.hip:
// Standard_glTF.shader's materials): the set-up (raster.hip's rules over interleaved vertices, on the helpers of raster_prims.h), the depth test of one fragment, the workspace layout, the varyings of a vertex, the
// texture taps and the checks of the entry points.  Those checks are written once, host-only, at the end of this file: surf_workspace_why (band, workspace
// alignment, descriptor slots) for every entry that takes the workspace, surf_draw_prologue (every check the draw entries share, their matrices and their
// grid with its slices) and surf_resolve_why (the three resolves).  The launches behind them are written once as well: surf_draw_launch for every draw entry
// that takes the tables, surf_resolve_launch for the resolves.  An entry keeps the checks that are its own; surf_refuse puts the entry's name in front of the
// reason.  The resolve kernels' body and the search for a pixel's draw are surface_resolve_body.h's.
#pragma once
#include <type_traits>
#include "common.h"
#include "sampling.h"
#include "texel_pass.h"
#include "raster_prims.h"

#define SURF_SMALL_BOX 64   // pixels a lane fills on its own
#define SURF_VERTEX_FLOATS 18
#define SURF_INSTANCE_FLOATS 24
#define SURF_HEADER_BYTES 64
#define SURF_TABLE_BYTES 1024
#define SURF_MAX_DRAWS (1u << 20)
#define SURF_SLICE_LANES 262144ull
#define SURF_SLICES_MAX 256ull

struct SurfHeader { uint32_t maxDraws, rows, width, fbRowBegin; uint32_t pad[12]; };
struct SurfSrgb { float v[256]; };

// where the three vertices of a set-up triangle came from: vertex k is source vertex I[k], or -- cut[k] -- the point I[k] + (O[k] - I[k]) * t[k] of an
// edge the near plane cut; w[k] is its clip w
struct SurfSrc { uint32_t I[3], O[3]; float t[3], w[3]; bool cut[3]; };

// raster_setup of raster.hip from the clip positions c[0..2] of the triangle's vertices v0, v1, v2 on: the near-plane cut, the snap, the cull and the box;
// rows [rowBegin, rowEnd) of the frame only.  S reports the vertices' sources for the varyings (dead code where it is not read).
// PIXEL_BOX (default false: the box of the pixel CENTRES inside the bounding box, as ever): the box of every pixel the bounding box touches, for the
// multisampled walk of surface_fill_msaa.h, whose samples lie anywhere in a pixel -- a triangle that holds no centre is valid there.
template <bool PIXEL_BOX = false>
__device__ __forceinline__ SurfTri surface_setup_clip(float4 (&c)[3], const uint32_t v0, const uint32_t v1, const uint32_t v2, int W, int H, int rowBegin, int rowEnd,
                                                      bool cullBack, int part, bool& hasSecond, SurfSrc& S)
{
    SurfTri t;
    t.valid = false;
    hasSecond = false;
    S.I[0] = v0; S.I[1] = v1; S.I[2] = v2;
    S.O[0] = v0; S.O[1] = v1; S.O[2] = v2;
    S.t[0] = S.t[1] = S.t[2] = 0.0f;
    S.cut[0] = S.cut[1] = S.cut[2] = false;
    const float d0 = c[0].w - c[0].z, d1 = c[1].w - c[1].z, d2 = c[2].w - c[2].z;
    const int mask = (d0 >= 0.0f ? 1 : 0) | (d1 >= 0.0f ? 2 : 0) | (d2 >= 0.0f ? 4 : 0);
    if (mask == 0) return t;
    if (mask != 7) {
        const bool one = (mask & (mask - 1)) == 0;
        const int r = one ? (mask == 1 ? 0 : (mask == 2 ? 1 : 2)) : (mask == 6 ? 1 : (mask == 5 ? 2 : 0)); // the rotation that brings A to the front
        const float4 A = r == 0 ? c[0] : (r == 1 ? c[1] : c[2]), B = r == 0 ? c[1] : (r == 1 ? c[2] : c[0]), C = r == 0 ? c[2] : (r == 1 ? c[0] : c[1]);
        const float dA = r == 0 ? d0 : (r == 1 ? d1 : d2), dB = r == 0 ? d1 : (r == 1 ? d2 : d0), dC = r == 0 ? d2 : (r == 1 ? d0 : d1);
        const uint32_t iA = r == 0 ? v0 : (r == 1 ? v1 : v2), iB = r == 0 ? v1 : (r == 1 ? v2 : v0), iC = r == 0 ? v2 : (r == 1 ? v0 : v1);
        S.I[0] = iA; S.O[0] = iA;
        if (one) {
            if (part) return t;
            c[0] = A; c[1] = surf_cut(A, dA, B, dB, S.t[1]); c[2] = surf_cut(A, dA, C, dC, S.t[2]);
            S.I[1] = iA; S.O[1] = iB; S.cut[1] = true;
            S.I[2] = iA; S.O[2] = iC; S.cut[2] = true;
        } else {
            float tBC;
            const float4 BC = surf_cut(B, dB, C, dC, tBC);
            hasSecond = true;
            c[0] = A;
            if (part == 0) {
                c[1] = B; c[2] = BC;
                S.I[1] = iB; S.O[1] = iB;
                S.I[2] = iB; S.O[2] = iC; S.t[2] = tBC; S.cut[2] = true;
            } else {
                c[1] = BC; c[2] = surf_cut(A, dA, C, dC, S.t[2]);
                S.I[1] = iB; S.O[1] = iC; S.t[1] = tBC; S.cut[1] = true;
                S.I[2] = iA; S.O[2] = iC; S.cut[2] = true;
            }
        }
    } else if (part) return t;
    long long X[3], Y[3];
    float Z[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 clip = c[k];
        if (!(clip.w > 0.0f)) return t;
        const float nx = clip.x / clip.w, ny = clip.y / clip.w, nz = clip.z / clip.w;
        const float xf = (nx + 1.0f) * ((float)W * 0.5f);
        const float yf = (ny + 1.0f) * ((float)H * -0.5f) + (float)H;
        const float sx = xf * 256.0f, sy = yf * 256.0f;
        if (!(fabsf(sx) < 1.0e9f) || !(fabsf(sy) < 1.0e9f)) return t;
        X[k] = (long long)rintf(sx); Y[k] = (long long)rintf(sy); Z[k] = nz;
        S.w[k] = clip.w;
    }
    const long long area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]);
    if (area2 == 0) return t;
    if (cullBack && area2 > 0) return t; // Vulkan's signed area is -area2 / 2, front = counter-clockwise = positive (see the oracle)
    if (area2 < 0) { // the winding swap takes the varyings' sources along
        long long s = X[1]; X[1] = X[2]; X[2] = s; s = Y[1]; Y[1] = Y[2]; Y[2] = s; const float z = Z[1]; Z[1] = Z[2]; Z[2] = z;
        const uint32_t i = S.I[1]; S.I[1] = S.I[2]; S.I[2] = i; const uint32_t o = S.O[1]; S.O[1] = S.O[2]; S.O[2] = o;
        const float tt = S.t[1]; S.t[1] = S.t[2]; S.t[2] = tt; const float w = S.w[1]; S.w[1] = S.w[2]; S.w[2] = w;
        const bool cu = S.cut[1]; S.cut[1] = S.cut[2]; S.cut[2] = cu;
    }
    t.x0 = X[0]; t.y0 = Y[0]; t.x1 = X[1]; t.y1 = Y[1]; t.x2 = X[2]; t.y2 = Y[2];
    t.z0 = Z[0]; t.z1 = Z[1]; t.z2 = Z[2];
    const long long minx = min(X[0], min(X[1], X[2])), maxx = max(X[0], max(X[1], X[2]));
    const long long miny = min(Y[0], min(Y[1], Y[2])), maxy = max(Y[0], max(Y[1], Y[2]));
    long long i0 = surf_floor_div256(minx - 128 + 255), i1 = surf_floor_div256(maxx - 128);
    long long j0 = surf_floor_div256(miny - 128 + 255), j1 = surf_floor_div256(maxy - 128);
    if constexpr (PIXEL_BOX) { i0 = surf_floor_div256(minx); i1 = surf_floor_div256(maxx); j0 = surf_floor_div256(miny); j1 = surf_floor_div256(maxy); }
    if (i0 < 0) i0 = 0;
    if (j0 < rowBegin) j0 = rowBegin;
    if (i1 > W - 1) i1 = W - 1;
    if (j1 > rowEnd - 1) j1 = rowEnd - 1;
    if (i1 < i0 || j1 < j0) return t;
    t.i0 = (int)i0; t.i1 = (int)i1; t.j0 = (int)j0; t.j1 = (int)j1;
    t.valid = true;
    return t;
}

// hasView form: clip = projection * (view * (model * position)) (DepthOnly.shader:51 == Standard.shader:131) over interleaved vertices
template <bool PIXEL_BOX = false>
__device__ __forceinline__ SurfTri surface_setup(const Mat4& P, const Mat4& V, const float* __restrict__ model, const float* __restrict__ vertices,
                                                 const uint32_t* __restrict__ tri, int W, int H, int rowBegin, int rowEnd, bool cullBack, int part, bool& hasSecond,
                                                 SurfSrc& S)
{
    float4 c[3];
    const uint32_t v0 = tri[0], v1 = tri[1], v2 = tri[2];
    Mat4 M;
#pragma unroll
    for (int q = 0; q < 16; q++) M.m[q] = model[q];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float* p = vertices + SURF_VERTEX_FLOATS * (size_t)(k == 0 ? v0 : (k == 1 ? v1 : v2)) + 2;
        const float4 a = glsl_mul(M, p[0], p[1], p[2], 1.0f);
        const float4 bq = glsl_mul(V, a.x, a.y, a.z, a.w);
        c[k] = glsl_mul(P, bq.x, bq.y, bq.z, bq.w);
    }
    return surface_setup_clip<PIXEL_BOX>(c, v0, v1, v2, W, H, rowBegin, rowEnd, cullBack, part, hasSecond, S);
}

// one matrix: clip = LM * position (a caster draw: LM = lightMatrix * model, raster.hip's form without a view)
__device__ __forceinline__ SurfTri surface_setup_matrix(const Mat4& LM, const float* __restrict__ vertices, const uint32_t* __restrict__ tri, int W, int H, int rowBegin,
                                                        int rowEnd, bool cullBack, int part, bool& hasSecond, SurfSrc& S)
{
    float4 c[3];
    const uint32_t v0 = tri[0], v1 = tri[1], v2 = tri[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float* p = vertices + SURF_VERTEX_FLOATS * (size_t)(k == 0 ? v0 : (k == 1 ? v1 : v2)) + 2;
        c[k] = glsl_mul(LM, p[0], p[1], p[2], 1.0f);
    }
    return surface_setup_clip(c, v0, v1, v2, W, H, rowBegin, rowEnd, cullBack, part, hasSecond, S);
}

// the depth test of one fragment, GreaterOrEqual in primitive order: the larger key wins.  A relaxed atomic load first (other waves run atomicMax on the
// same word): a fragment that has already lost never reaches the atomic, and a stale value can only be SMALLER than the key now stored, so no winner is
// dropped.
__device__ __forceinline__ void surf_fragment(unsigned long long* p, float z, unsigned int orderPlus1)
{
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | orderPlus1;
    if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, key);
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------------------
struct SurfWorkspace { SurfHeader* header; float* srgb; unsigned long long* keys; SailorSurfaceDraw* draws; };
static __host__ __device__ __forceinline__ SurfWorkspace surf_workspace(void* base, size_t pixels)
{
    SurfWorkspace w;
    char* b = reinterpret_cast<char*>(base);
    w.header = reinterpret_cast<SurfHeader*>(b);
    w.srgb = reinterpret_cast<float*>(b + SURF_HEADER_BYTES);
    w.keys = reinterpret_cast<unsigned long long*>(b + SURF_HEADER_BYTES + SURF_TABLE_BYTES);
    w.draws = reinterpret_cast<SailorSurfaceDraw*>(b + SURF_HEADER_BYTES + SURF_TABLE_BYTES + pixels * 8);
    return w;
}

// the bilinear Repeat fetch of one width x height RGBA8 level; SRGB decodes r, g, b per tap through the table before the filter
__device__ __forceinline__ float4 surf_texels_fetch(const uint32_t* __restrict__ texels, int width, int height, uint32_t flags, const float* __restrict__ srgb, float u,
                                                    float v)
{
    if (!(flags & SAILOR_TEXTURE_SRGB)) return bilinear_repeat_rgba8(texels, width, height, u, v);
    const RepeatTap X = repeat_tap(width, u), Y = repeat_tap(height, v);
    const uint32_t a = texels[Y.i0 * width + X.i0], c = texels[Y.i0 * width + X.i1], e = texels[Y.i1 * width + X.i0], f = texels[Y.i1 * width + X.i1];
    float4 r;
    r.x = lerp2(srgb[a & 255u], srgb[c & 255u], srgb[e & 255u], srgb[f & 255u], X.a, Y.a);
    r.y = lerp2(srgb[(a >> 8) & 255u], srgb[(c >> 8) & 255u], srgb[(e >> 8) & 255u], srgb[(f >> 8) & 255u], X.a, Y.a);
    r.z = lerp2(srgb[(a >> 16) & 255u], srgb[(c >> 16) & 255u], srgb[(e >> 16) & 255u], srgb[(f >> 16) & 255u], X.a, Y.a);
    r.w = lerp2(unorm8(a >> 24), unorm8(c >> 24), unorm8(e >> 24), unorm8(f >> 24), X.a, Y.a);
    return r;
}

// texture(textureSamplers[index], uv): base level, bilinear, Repeat (the implicit level of detail: surface_lod.h)
__device__ __forceinline__ float4 surf_texture(const SailorTextureDesc* __restrict__ textures, uint32_t numTextures, uint32_t index, const float* __restrict__ srgb,
                                               float u, float v)
{
    const SailorTextureDesc d = textures[index < numTextures ? index : 0u];
    if (!d.texels || d.width <= 0 || d.height <= 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return surf_texels_fetch(d.texels, d.width, d.height, d.flags, srgb, u, v);
}

// the alpha of texture(textureSamplers[index], uv) alone: surf_texture's .w (alpha is never sRGB-decoded, so both of its branches compute exactly this)
__device__ __forceinline__ float surf_texture_alpha(const uint32_t* __restrict__ texels, int width, int height, float u, float v)
{
    if (!texels || width <= 0 || height <= 0) return 0.0f;
    const RepeatTap X = repeat_tap(width, u), Y = repeat_tap(height, v);
    const uint32_t a = texels[Y.i0 * width + X.i0], c = texels[Y.i0 * width + X.i1], e = texels[Y.i1 * width + X.i0], f = texels[Y.i1 * width + X.i1];
    return lerp2(unorm8(a >> 24), unorm8(c >> 24), unorm8(e >> 24), unorm8(f >> 24), X.a, Y.a);
}

// varying c of source vertex v under the instance's model m (Standard.shader:128-138): 0-1 texcoord, 2-4 worldPosition = (model * vec4(p, 1)).xyz / .w,
// 5-8 color, 9-17 tangentBasis = mat3(model) * mat3(inTangent, inBitangent, inNormal), column by column.  c is a compile-time constant where it is called.
__device__ __forceinline__ float surf_varying(const float* __restrict__ v, const float* __restrict__ m, int c)
{
    if (c < 2) return v[c];
    if (c < 5) {
        const int r = c - 2;
        const float x = v[2], y = v[3], z = v[4];
        const float a = ((m[r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * 1.0f;
        const float w = ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * 1.0f;
        return a / w;
    }
    if (c < 9) return v[14 + (c - 5)];
    const int col = (c - 9) / 3, r = (c - 9) % 3;
    const float* __restrict__ a = v + (col == 0 ? 8 : (col == 1 ? 11 : 5));
    return (m[r] * a[0] + m[4 + r] * a[1]) + m[8 + r] * a[2];
}

// the matrix under the tangent basis, three columns of three: mat3(model) (Standard.shader:138) or transpose(inverse(mat3(model))) in glm's form
// (Standard_glTF.shader:136; the header's rule 4), one rounding per written operation
__device__ __forceinline__ void surf_basis_matrix(const float* __restrict__ m, bool gltf, float n[9])
{
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10];
    if (!gltf) {
        n[0] = m00; n[1] = m01; n[2] = m02; n[3] = m10; n[4] = m11; n[5] = m12; n[6] = m20; n[7] = m21; n[8] = m22;
        return;
    }
    const float c00 = m11 * m22 - m21 * m12, c01 = m01 * m22 - m21 * m02, c02 = m01 * m12 - m11 * m02;
    const float det = (m00 * c00 - m10 * c01) + m20 * c02;
    const float oneOverDet = 1.0f / det;
    // N[c][r] = I[r][c]: column c of N is row c of the inverse
    n[0] = c00 * oneOverDet;                        // I00
    n[1] = -(m10 * m22 - m20 * m12) * oneOverDet;   // I10
    n[2] = (m10 * m21 - m20 * m11) * oneOverDet;    // I20
    n[3] = -c01 * oneOverDet;                       // I01
    n[4] = (m00 * m22 - m20 * m02) * oneOverDet;    // I11
    n[5] = -(m00 * m21 - m20 * m01) * oneOverDet;   // I21
    n[6] = c02 * oneOverDet;                        // I02
    n[7] = -(m00 * m12 - m10 * m02) * oneOverDet;   // I12
    n[8] = (m00 * m11 - m10 * m01) * oneOverDet;    // I22
}

// surf_varying with the tangent basis (c = 9..17) under the matrix n of surf_basis_matrix
__device__ __forceinline__ float surf_varying_basis(const float* __restrict__ v, const float* __restrict__ m, const float n[9], int c)
{
    if (c < 9) return surf_varying(v, m, c);
    const int col = (c - 9) / 3, r = (c - 9) % 3;
    const float* __restrict__ a = v + (col == 0 ? 8 : (col == 1 ? 11 : 5));
    return (n[r] * a[0] + n[3 + r] * a[1]) + n[6 + r] * a[2];
}

// ---- what every entry point checks ------------------------------------------------------------------------------------------------------------------
// last_error = "<the entry's name>: <what>"
static int surf_refuse(SailorHipContext* ctx, const char* who, const char* what)
{
    if (ctx) ctx->lastError = std::string(who) + ": " + what;
    return SAILOR_HIP_ERR_INVALID_ARGUMENT;
}
static bool surf_band_ok(int32_t width, int32_t height, const SailorBand* band)
{
    return band && extent_ok(width, height) && sailor_hip_band_is_valid(width, height, band) == 1 && band->fbRowCount > 0;
}
static size_t surf_fixed_bytes(int32_t width, const SailorBand* band)
{
    return (size_t)SURF_HEADER_BYTES + SURF_TABLE_BYTES + (size_t)band->fbRowCount * width * 8;
}
// the descriptor slots a workspace of `bytes` holds
static uint32_t surf_max_draws(int32_t width, const SailorBand* band, size_t bytes)
{
    const size_t fixed = surf_fixed_bytes(width, band);
    if (bytes < fixed + sizeof(SailorSurfaceDraw)) return 0;
    const size_t n = (bytes - fixed) / sizeof(SailorSurfaceDraw);
    return (uint32_t)(n < SURF_MAX_DRAWS ? n : SURF_MAX_DRAWS);
}
// The band is valid for the frame, the workspace is 16-byte aligned and holds at least one descriptor slot: why not, or NULL.  `split`: an entry that
// writes the workspace tells a bad pointer from a small workspace; one that only reads it has a single message for both.
static const char* surf_workspace_why(int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace, size_t workspaceBytes, bool split,
                                      uint32_t* maxDraws = nullptr)
{
    if (!surf_band_ok(width, height, band)) return "the band is not valid for the frame";
    const uint32_t n = surf_max_draws(width, band, workspaceBytes);
    if (maxDraws) *maxDraws = n;
    if (split && !aligned(dWorkspace, 16)) return "the workspace is NULL or not 16-byte aligned";
    if (split && n == 0) return "the workspace is too small";
    if (!aligned(dWorkspace, 16) || n == 0) return "the workspace is NULL, misaligned or too small";
    return nullptr;
}
// the slices of a draw of `lanes` triangles or segments (see k_surface_visibility): about SURF_SLICE_LANES lanes in flight for a draw of few, one slice from
// that many on
static unsigned surf_slices(unsigned long long lanes)
{
    const unsigned long long want = lanes ? SURF_SLICE_LANES / lanes : 1;
    return (unsigned)(want < 1 ? 1 : (want > SURF_SLICES_MAX ? SURF_SLICES_MAX : want));
}
static bool surf_tables_ok(const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures)
{
    return dMaterials && dTextures && numMaterials != 0 && numTextures != 0;
}

// What the draw entries (sailor_hip_surface_draw and, through surf_draw_launch, those that take the tables) check, in one order, and what their launches share: the two matrices,
// the lanes of the draw and the grid.  `allowed` = the flag bits the entry accepts, needGltf = SAILOR_SURFACE_GLTF has to be among the draw's, `tables` =
// surf_tables_ok of the entry's tables (read under ALPHA_CUTOUT only); dCommand = NULL for a direct entry, the address of the indirect entry's command
// pointer: that entry checks the command and dInstanceIds as well, and its lanes are the CAPACITY's (the count is not known on the host).
struct SurfDrawSetup { Mat4 P, V; unsigned long long total; dim3 grid; };
static int surf_draw_prologue(SailorHipContext* ctx, const char* who, uint32_t allowed, bool needGltf, const SailorDrawIndexedIndirectData* const* dCommand,
                              const SailorUboFrameData* frame, const SailorSurfaceDraw* draw, const SailorPerInstanceData* dInstances, bool tables, uint32_t drawIndex,
                              int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace, size_t workspaceBytes, SurfDrawSetup& s)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!frame || !draw) return surf_refuse(ctx, who, "frame or draw is NULL");
    if (dCommand && !aligned(*dCommand, 4)) return surf_refuse(ctx, who, "the command is NULL or not 4-byte aligned");
    uint32_t maxDraws = 0;
    if (const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, true, &maxDraws)) return surf_refuse(ctx, who, why);
    if (drawIndex >= maxDraws) return surf_refuse(ctx, who, "drawIndex is beyond the workspace's descriptor slots");
    if (draw->flags & ~allowed) return surf_refuse(ctx, who, "unknown flags");
    if (needGltf && !(draw->flags & SAILOR_SURFACE_GLTF)) return surf_refuse(ctx, who, "the draw does not carry SAILOR_SURFACE_GLTF");
    if (dCommand && draw->dInstanceIds) return surf_refuse(ctx, who, "dInstanceIds must be NULL (the instances are firstInstance + d of the command)");
    if ((draw->flags & SAILOR_SURFACE_ALPHA_CUTOUT) && !tables) return surf_refuse(ctx, who, "ALPHA_CUTOUT needs materials and textures");
    s.total = (unsigned long long)draw->numDrawn * draw->numTriangles;
    if (s.total && (!draw->dVertices || !draw->dIndices || !dInstances)) return surf_refuse(ctx, who, "a vertex, index or instance buffer is NULL");
    if (s.total > 0x7FFFFFFFull || (unsigned long long)draw->primBase + 2ull * s.total >= 0xFFFFFFFFull)
        return surf_refuse(ctx, who, dCommand ? "primBase + the capacity's primitives reaches 2^32 - 1" : "primBase + the draw's primitives reaches 2^32 - 1");
    memcpy(s.P.m, frame->projection, 64);
    memcpy(s.V.m, frame->view, 64);
    s.grid = dim3((unsigned)(s.total ? (s.total + 255) / 256 : 1), surf_slices(s.total)); // (an empty draw still leaves its descriptor)
    return SAILOR_HIP_OK;
}

// Every draw entry that takes the tables (_draw_masked, _draw_gltf, _draw_indirect, _draw_lod, _draw_indirect_lod, _peel_draw[_gltf], _bucket_draw[_gltf], _msaa_draw[_gltf]), in
// the one order that can be observed (a refusal launches nothing): surf_draw_prologue, the entry's own refusals, hipSetDevice, the launch.  kernelGltf (or
// NULL; its type is `kernel`'s, not deduced) is launched instead of `kernel` for a draw that carries SAILOR_SURFACE_GLTF.  command = SurfNoCommand(), or the indirect entry's command and record
// count, which its kernels take after the draw.  extra() = the status of the entry's own refusals, made through surf_refuse (SAILOR_HIP_OK: none); tail = what
// the kernel takes after the workspace.
struct SurfNoCommand {};
struct SurfCommand { const SailorDrawIndexedIndirectData* dCommand; uint32_t numInstanceRecords; };
static int surf_no_refusals() { return SAILOR_HIP_OK; }
template <typename K, typename C, typename Extra, typename... Tail>
static int surf_draw_launch(SailorHipContext* ctx, const char* who, uint32_t allowed, bool needGltf, K kernel, const char* kernelName, typename std::common_type<K>::type kernelGltf,
                            const char* kernelGltfName, const C command, Extra extra, const SailorUboFrameData* frame, const SailorSurfaceDraw* draw,
                            const SailorPerInstanceData* dInstances, const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures,
                            uint32_t numTextures, uint32_t drawIndex, int32_t width, int32_t height, const SailorBand* band, void* dWorkspace, size_t workspaceBytes, Tail... tail)
{
    constexpr bool indirect = std::is_same<C, SurfCommand>::value;
    const SailorDrawIndexedIndirectData* const* dCommand = nullptr;
    if constexpr (indirect) dCommand = &command.dCommand;
    SurfDrawSetup s;
    if (const int st = surf_draw_prologue(ctx, who, allowed, needGltf, dCommand, frame, draw, dInstances, surf_tables_ok(dMaterials, numMaterials, dTextures, numTextures), drawIndex,
                                          width, height, band, dWorkspace, workspaceBytes, s))
        return st;
    if (const int st = extra()) return st;
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    const bool gltf = kernelGltf && (draw->flags & SAILOR_SURFACE_GLTF);
    const auto launch = [&](auto... afterDraw) {
        sailor_launch(ctx, gltf ? kernelGltf : kernel, s.grid, dim3(256), s.P, s.V, *draw, afterDraw..., reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials,
                      dTextures, numTextures, drawIndex, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace, tail...);
    };
    if constexpr (indirect) launch(reinterpret_cast<const uint32_t*>(command.dCommand), command.numInstanceRecords);
    else launch();
    SAILOR_CHECK_LAUNCH(ctx, gltf ? kernelGltfName : kernelName);
    return SAILOR_HIP_OK;
}

// What the three resolve entries check alike (`rest` = the instances are there and surf_tables_ok of the tables), and the matrices and the descriptor slots
// their kernels take: why not, or NULL
struct SurfResolveSetup { Mat4 P, V; uint32_t maxDraws; };
static const char* surf_resolve_why(const SailorUboFrameData* frame, bool rest, int32_t width, int32_t height, const SailorBand* band, const void* dWorkspace,
                                    size_t workspaceBytes, const float* dSurface, size_t planeStride, const float* dDepthOutOrNull, SurfResolveSetup& s)
{
    if (!frame || !rest) return "frame, instances, materials or textures missing";
    if (const char* why = surf_workspace_why(width, height, band, dWorkspace, workspaceBytes, false, &s.maxDraws)) return why;
    if (!aligned(dSurface, 16)) return "the surface is NULL or not 16-byte aligned";
    if (planeStride < (size_t)band->fbRowCount * width) return "planeStride is smaller than the band's rows x width";
    if (dDepthOutOrNull && !aligned(dDepthOutOrNull, 4)) return "the depth output is misaligned";
    memcpy(s.P.m, frame->projection, 64);
    memcpy(s.V.m, frame->view, 64);
    return nullptr;
}
// what _resolve_gltf and _resolve_lod check of their occlusion and emissive planes, after everything else; sailor_hip_surface_resolve has no such planes
static const char* surf_resolve_planes_why() { return nullptr; }
static const char* surf_resolve_planes_why(const float* dAoInOrNull, float* dAoOutOrNull, float4* dEmissive)
{
    if ((dAoInOrNull && !aligned(dAoInOrNull, 4)) || (dAoOutOrNull && !aligned(dAoOutOrNull, 4))) return "an occlusion plane is misaligned";
    if (!aligned(dEmissive, 16)) return "the emissive plane is NULL or not 16-byte aligned";
    return nullptr;
}
// The three resolve entries: the checks, hipSetDevice, the launch.  planes = what the kernel takes after the coverage: nothing, or (aoIn, aoOut, emissive).
template <typename K, typename... Planes>
static int surf_resolve_launch(SailorHipContext* ctx, const char* who, K kernel, const char* kernelName, const SailorUboFrameData* frame, const SailorPerInstanceData* dInstances,
                               const SailorMaterialData* dMaterials, uint32_t numMaterials, const SailorTextureDesc* dTextures, uint32_t numTextures, int32_t width, int32_t height,
                               const SailorBand* band, const void* dWorkspace, size_t workspaceBytes, float* dSurface, size_t planeStride, float* dDepthOutOrNull,
                               uint8_t* dCoverageOrNull, Planes... planes)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    SurfResolveSetup s;
    const char* why = surf_resolve_why(frame, dInstances && surf_tables_ok(dMaterials, numMaterials, dTextures, numTextures), width, height, band, dWorkspace, workspaceBytes,
                                       dSurface, planeStride, dDepthOutOrNull, s);
    if (!why) why = surf_resolve_planes_why(planes...);
    if (why) return surf_refuse(ctx, who, why);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, kernel, texel_grid(width, band->fbRowCount), dim3(256), s.P, s.V, reinterpret_cast<const float*>(dInstances), dMaterials, numMaterials, dTextures,
                  numTextures, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, s.maxDraws, dWorkspace, reinterpret_cast<float4*>(dSurface), planeStride,
                  dDepthOutOrNull, dCoverageOrNull, planes...);
    SAILOR_CHECK_LAUNCH(ctx, kernelName);
    return SAILOR_HIP_OK;
}
