// The RenderImGui node's pass: ImGuiUI.shader (`gl_Position = vec4(aPos * uScale + uTranslate, 0, 1)`, `fColor = inColor * texture(sTexture, inUV)`) under the
// material of Submodules/ImGuiApi.cpp:295-332 -- TriangleList, no depth test, no cull, EBlendMode::AlphaBlending -- as an ORDERED, atomic-free, tile-binned
// blender for gfx950.  include/sailor_hip.h has the pinned rules; tests/ui_ref.py restates them sequentially and the kernels are held to it bit for bit.
//
//   k_ui_scan    one block: the cumulative triangle counts of the commands (indexCount / 3 each, 0 for a range outside the index buffer), clamped to the
//                number of records the workspace holds, into the workspace.
//   k_ui_setup   a lane per triangle: its command by binary search over those counts, the index and vertex fetch, the vertex stage, the snap, the winding
//                swap, the pixel box cut to the command's scissor, the frame and the band's rows.  It writes the box (16 bytes, its own array: the blend's
//                bin test reads nothing else) and a 64-byte record: three snapped positions, three packed colours, three uvs.  A dropped or fully scissored
//                triangle gets an empty box.
//   k_ui_blend   a block of 256 per bin of 32 x 32 pixels of the band.  The block walks the commands in order; a command whose scissor misses the bin is
//                skipped with its whole triangle range.  Of the others it walks the boxes in chunks of 256 IN ORDER: a lane tests one box against the bin,
//                ballot + mbcnt compact the survivors into LDS preserving order.  Then each wave, for its own row of four 8 x 8 tiles, walks the LDS list in
//                order (all lanes read the same record: a broadcast), and a lane per pixel runs the box test, the edge functions, the top-left rule, the
//                varyings, the four texel taps and the blend on the pixel it keeps in registers.  Pixels are loaded when the bin's first record arrives and
//                stored once, after the last chunk, where a fragment touched them.  (A wave-uniform skip of a triangle whose box misses the wave's tiles was
//                built and measured: the branch waits for the box before the record's loads go out, and the pass was 2 to 4 % slower with it.  DESIGN.md.)
//
//                Every (float)byte / 255.0f of a colour or a texel comes from a table of the 256 quotients the block computes into LDS with that division.
//
// Order never depends on scheduling: a pixel belongs to one lane from the first triangle to the last.
#include "surface_common.h"

#define UI_BIN 32
#define UI_CHUNK 256
#define UI_HEADER_BYTES ((size_t)(SAILOR_UI_MAX_COMMANDS + 4) * 4)
// 0 computes every (float)byte / 255.0f where it is used instead of reading the block's table of the 256 quotients: for the measurement in DESIGN.md only
#ifndef SAILOR_UI_UNORM_TABLE
#define SAILOR_UI_UNORM_TABLE 1
#endif
// 0 walks every command's triangles in every bin: for the measurement in DESIGN.md only, never shipped
#ifndef SAILOR_UI_COMMAND_REJECT
#define SAILOR_UI_COMMAND_REJECT 1
#endif

// what follows the box: the snapped positions (|.| < 1e9, so they fit; area > 0 after the swap), the colours and uvs of the three vertices in that order
struct UiRecord { int x0, y0, x1, y1, x2, y2; uint32_t c0, c1, c2; float u0, v0, u1, v1, u2, v2; uint32_t pad; };
static_assert(sizeof(UiRecord) == 64, "UiRecord is four float4");

struct UiWorkspace { uint32_t* cum; int4* boxes; UiRecord* records; };
static __host__ __device__ __forceinline__ UiWorkspace ui_workspace(void* base, size_t numTriangles)
{
    UiWorkspace w;
    char* b = reinterpret_cast<char*>(base);
    w.cum = reinterpret_cast<uint32_t*>(b);
    w.boxes = reinterpret_cast<int4*>(b + UI_HEADER_BYTES);
    w.records = reinterpret_cast<UiRecord*>(b + UI_HEADER_BYTES + numTriangles * 16);
    return w;
}
static size_t ui_workspace_bytes(size_t numTriangles) { return UI_HEADER_BYTES + (numTriangles ? numTriangles : 1) * 80; }

struct UiDraw {
    const SailorVertexP2UV2C1* vertices;
    const void* indices;
    const SailorUiCommand* commands;
    uint32_t numVertices, numIndices, numCommands, numTriangles, indexBytes;
    float scaleX, scaleY, translateX, translateY;
};

// the triangles of a command as the kernels count them: none if its range leaves the index buffer
__device__ __forceinline__ uint32_t ui_command_triangles(const SailorUiCommand& c, uint32_t numIndices)
{
    return (unsigned long long)c.firstIndex + c.indexCount <= numIndices ? c.indexCount / 3u : 0u;
}

__global__ __launch_bounds__(256) void k_ui_scan(UiDraw d, void* __restrict__ workspace)
{
    __shared__ unsigned long long s_wave[4];
    const UiWorkspace ws = ui_workspace(workspace, d.numTriangles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long running = 0;
    if (tid == 0) ws.cum[0] = 0u;
    for (uint32_t base = 0; base < d.numCommands; base += 256) {
        const uint32_t c = base + tid;
        unsigned long long v = c < d.numCommands ? ui_command_triangles(d.commands[c], d.numIndices) : 0u;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) { // inclusive scan of the wave
            const unsigned long long o = __shfl_up(v, s, 64);
            if (lane >= s) v += o;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        unsigned long long before = running;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        const unsigned long long total = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        const unsigned long long sum = before + v;
        if (c < d.numCommands) ws.cum[c + 1] = (uint32_t)(sum < d.numTriangles ? sum : d.numTriangles);
        running += total;
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t ui_index(const void* __restrict__ indices, uint32_t indexBytes, unsigned long long at)
{
    return indexBytes == 2u ? (uint32_t)reinterpret_cast<const uint16_t*>(indices)[at] : reinterpret_cast<const uint32_t*>(indices)[at];
}

__global__ __launch_bounds__(256) void k_ui_setup(UiDraw d, int W, int H, int rowBegin, int rows, void* __restrict__ workspace)
{
    const UiWorkspace ws = ui_workspace(workspace, d.numTriangles);
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= d.numTriangles) return;
    int4 box = make_int4(1, 0, 1, 0); // i0, i1, j0, j1: empty
    UiRecord r;
    r.x0 = r.y0 = r.x1 = r.y1 = r.x2 = r.y2 = 0; r.c0 = r.c1 = r.c2 = 0u; r.u0 = r.v0 = r.u1 = r.v1 = r.u2 = r.v2 = 0.0f; r.pad = 0u;
    // the command: the last c with cum[c] <= t (commands without triangles repeat a count and are stepped over)
    uint32_t lo = 0, hi = d.numCommands; // cum[lo] <= t, answer in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (ws.cum[mid] <= t) lo = mid; else hi = mid;
    }
    if (t < ws.cum[lo + 1]) {
        const SailorUiCommand c = d.commands[lo];
        const unsigned long long at = (unsigned long long)c.firstIndex + 3ull * (t - ws.cum[lo]);
        bool ok = at + 2ull < d.numIndices;
        long long v[3] = {0, 0, 0};
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                v[k] = (long long)c.vertexOffset + (long long)ui_index(d.indices, d.indexBytes, at + k);
                ok = ok && v[k] >= 0 && v[k] < (long long)d.numVertices;
            }
        }
        if (ok) {
            long long X[3], Y[3];
            uint32_t C[3];
            float U[3], V[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const SailorVertexP2UV2C1 p = d.vertices[v[k]];
                const float nx = p.position[0] * d.scaleX + d.translateX, ny = p.position[1] * d.scaleY + d.translateY;
                const float xf = (nx + 1.0f) * ((float)W * 0.5f), yf = (ny + 1.0f) * ((float)H * 0.5f);
                const float sx = xf * 256.0f, sy = yf * 256.0f;
                if (!(fabsf(sx) < 1.0e9f) || !(fabsf(sy) < 1.0e9f)) ok = false;
                X[k] = ok ? (long long)rintf(sx) : 0; Y[k] = ok ? (long long)rintf(sy) : 0;
                C[k] = p.color; U[k] = p.uv[0]; V[k] = p.uv[1];
            }
            const long long area2 = surf_edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
            if (ok && area2 != 0) {
                if (area2 < 0) { // the winding swap takes colour and uv along
                    long long s = X[1]; X[1] = X[2]; X[2] = s; s = Y[1]; Y[1] = Y[2]; Y[2] = s;
                    const uint32_t cc = C[1]; C[1] = C[2]; C[2] = cc;
                    float f = U[1]; U[1] = U[2]; U[2] = f; f = V[1]; V[1] = V[2]; V[2] = f;
                }
                const long long minx = min(X[0], min(X[1], X[2])), maxx = max(X[0], max(X[1], X[2]));
                const long long miny = min(Y[0], min(Y[1], Y[2])), maxy = max(Y[0], max(Y[1], Y[2]));
                long long i0 = surf_floor_div256(minx - 128 + 255), i1 = surf_floor_div256(maxx - 128);
                long long j0 = surf_floor_div256(miny - 128 + 255), j1 = surf_floor_div256(maxy - 128);
                // the scissor, the frame, the band's rows
                const long long sx0 = c.scissor[0], sy0 = c.scissor[1], sx1 = sx0 + c.scissor[2], sy1 = sy0 + c.scissor[3]; // [s0, s1)
                i0 = max(i0, max(sx0, 0ll)); i1 = min(i1, min(sx1, (long long)W) - 1);
                j0 = max(j0, max(sy0, (long long)rowBegin)); j1 = min(j1, min(sy1, (long long)rowBegin + rows) - 1);
                if (i0 <= i1 && j0 <= j1) {
                    box = make_int4((int)i0, (int)i1, (int)j0, (int)j1);
                    r.x0 = (int)X[0]; r.y0 = (int)Y[0]; r.x1 = (int)X[1]; r.y1 = (int)Y[1]; r.x2 = (int)X[2]; r.y2 = (int)Y[2];
                    r.c0 = C[0]; r.c1 = C[1]; r.c2 = C[2];
                    r.u0 = U[0]; r.v0 = V[0]; r.u1 = U[1]; r.v1 = V[1]; r.u2 = U[2]; r.v2 = V[2];
                }
            }
        }
    }
    ws.boxes[t] = box;
    float4* __restrict__ out = reinterpret_cast<float4*>(ws.records + t);
    const float4* in = reinterpret_cast<const float4*>(&r);
    out[0] = in[0]; out[1] = in[1]; out[2] = in[2]; out[3] = in[3];
}

struct UiLdsRecord { int4 box; UiRecord r; }; // 80 bytes

__device__ __forceinline__ float ui_mix(float a0, float a1, float a2, float l0, float l1, float l2) { return (a0 * l0 + a1 * l1) + a2 * l2; }

// (float)byte / 255.0f: from the block's table (k_ui_blend fills it with exactly this quotient, so the bits are the division's), or computed
#if SAILOR_UI_UNORM_TABLE
#define UI_UNORM(table, byte) ((table)[(byte)])
#else
#define UI_UNORM(table, byte) unorm8(byte)
#endif

// bilinear_repeat_rgba8 of sampling.h -- the same taps (repeat_tap), the same filter (lerp2), the same channel order -- with the texels' bytes through UI_UNORM
__device__ __forceinline__ float4 ui_texture(const float* unorm, const uint32_t* __restrict__ tex, int W, int H, float u, float v)
{
    const RepeatTap X = repeat_tap(W, u), Y = repeat_tap(H, v);
    const uint32_t a = tex[Y.i0 * W + X.i0], c = tex[Y.i0 * W + X.i1], d = tex[Y.i1 * W + X.i0], e = tex[Y.i1 * W + X.i1];
    float4 r;
    r.x = lerp2(UI_UNORM(unorm, a & 255u), UI_UNORM(unorm, c & 255u), UI_UNORM(unorm, d & 255u), UI_UNORM(unorm, e & 255u), X.a, Y.a);
    r.y = lerp2(UI_UNORM(unorm, (a >> 8) & 255u), UI_UNORM(unorm, (c >> 8) & 255u), UI_UNORM(unorm, (d >> 8) & 255u), UI_UNORM(unorm, (e >> 8) & 255u), X.a, Y.a);
    r.z = lerp2(UI_UNORM(unorm, (a >> 16) & 255u), UI_UNORM(unorm, (c >> 16) & 255u), UI_UNORM(unorm, (d >> 16) & 255u), UI_UNORM(unorm, (e >> 16) & 255u), X.a, Y.a);
    r.w = lerp2(UI_UNORM(unorm, a >> 24), UI_UNORM(unorm, c >> 24), UI_UNORM(unorm, d >> 24), UI_UNORM(unorm, e >> 24), X.a, Y.a);
    return r;
}

// one fragment onto the pixel a lane keeps: src = colour * texel, then the blend of VulkanPipileneStates.cpp:245-246
__device__ __forceinline__ void ui_fragment(const UiRecord& r, const float* unorm, const uint32_t* __restrict__ texels, int texW, int texH, float l0, float l1, float l2,
                                            float4& dst)
{
    const float cr = ui_mix(UI_UNORM(unorm, r.c0 & 255u), UI_UNORM(unorm, r.c1 & 255u), UI_UNORM(unorm, r.c2 & 255u), l0, l1, l2);
    const float cg = ui_mix(UI_UNORM(unorm, (r.c0 >> 8) & 255u), UI_UNORM(unorm, (r.c1 >> 8) & 255u), UI_UNORM(unorm, (r.c2 >> 8) & 255u), l0, l1, l2);
    const float cb = ui_mix(UI_UNORM(unorm, (r.c0 >> 16) & 255u), UI_UNORM(unorm, (r.c1 >> 16) & 255u), UI_UNORM(unorm, (r.c2 >> 16) & 255u), l0, l1, l2);
    const float ca = ui_mix(UI_UNORM(unorm, r.c0 >> 24), UI_UNORM(unorm, r.c1 >> 24), UI_UNORM(unorm, r.c2 >> 24), l0, l1, l2);
    const float u = ui_mix(r.u0, r.u1, r.u2, l0, l1, l2), v = ui_mix(r.v0, r.v1, r.v2, l0, l1, l2);
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (texW > 0) t = ui_texture(unorm, texels, texW, texH, u, v); // (texW == 0: a descriptor without texels)
    const float sr = cr * t.x, sg = cg * t.y, sb = cb * t.z, sa = ca * t.w;
    const float om = 1.0f - sa;
    dst.x = sr * sa + dst.x * om;
    dst.y = sg * sa + dst.y * om;
    dst.z = sb * sa + dst.z * om;
    dst.w = sa * sa - dst.w * om;
}

__global__ __launch_bounds__(256) void k_ui_blend(const SailorUiCommand* __restrict__ commands, uint32_t numCommands, uint32_t numTriangles,
                                                  const uint32_t* __restrict__ texels, int texW, int texH, int W, int rowBegin, int rows,
                                                  const void* __restrict__ workspace, float4* __restrict__ target)
{
    __shared__ UiLdsRecord s_list[UI_CHUNK];
    __shared__ int s_count[4];
    __shared__ float s_unorm[256];
    const UiWorkspace ws = ui_workspace(const_cast<void*>(workspace), numTriangles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_unorm[tid] = unorm8((uint32_t)tid); // the 256 quotients every colour and texel byte is looked up in (first read behind the chunk's barriers)
    // the bin (frame coordinates), the wave's row of tiles, the lane's pixel of each of its four tiles
    const int bi0 = (int)blockIdx.x * UI_BIN, bj0 = rowBegin + (int)blockIdx.y * UI_BIN;
    const int bi1 = min(bi0 + UI_BIN, W) - 1, bj1 = min(bj0 + UI_BIN, rowBegin + rows) - 1;
    const int wj0 = bj0 + wave * 8;
    const int pi = bi0 + (lane & 7), pj = wj0 + (lane >> 3);
    float4 acc0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), acc1 = acc0, acc2 = acc0, acc3 = acc0; // (named, not an array: the tile loop below is a real loop)
    unsigned touched = 0u;
    bool loaded = false;
    float4* __restrict__ row = target + (size_t)(pj - rowBegin) * W + pi; // the lane's pixel of tile 0 (dereferenced only inside the bin)

    for (uint32_t c = 0; c < numCommands; c++) {
        uint32_t t0 = ws.cum[c], t1 = ws.cum[c + 1];
        if (t1 > numTriangles) t1 = numTriangles; // (k_ui_scan has clamped them: a bound of its own for the loads below)
        if (t0 >= t1) continue;
#if SAILOR_UI_COMMAND_REJECT
        {
            const SailorUiCommand cmd = commands[c];
            const long long sx0 = cmd.scissor[0], sy0 = cmd.scissor[1], sx1 = sx0 + cmd.scissor[2], sy1 = sy0 + cmd.scissor[3];
            if (sx1 <= bi0 || sx0 > bi1 || sy1 <= bj0 || sy0 > bj1) continue; // block-uniform: the command's whole triangle range
        }
#endif
        for (uint32_t base = t0; base < t1; base += UI_CHUNK) {
            const uint32_t t = base + (uint32_t)tid;
            int4 box = make_int4(1, 0, 1, 0);
            if (t < t1) box = ws.boxes[t];
            const bool hit = box.x <= box.y && box.x <= bi1 && box.y >= bi0 && box.z <= bj1 && box.w >= bj0;
            const unsigned long long mask = __ballot(hit);
            if (lane == 0) s_count[wave] = __popcll(mask);
            __syncthreads(); // (also: every wave has finished the previous list)
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) { const int n = s_count[w]; total += n; if (w < wave) before += n; }
            if (total == 0) { __syncthreads(); continue; }
            if (hit) {
                const int at = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                const float4* __restrict__ in = reinterpret_cast<const float4*>(ws.records + t);
                float4* out = reinterpret_cast<float4*>(&s_list[at]);
                out[0] = make_float4(__int_as_float(box.x), __int_as_float(box.y), __int_as_float(box.z), __int_as_float(box.w));
                out[1] = in[0]; out[2] = in[1]; out[3] = in[2]; out[4] = in[3];
            }
            if (!loaded) { // the bin's first records: fetch the pixels the lane keeps
                loaded = true;
                if (pj <= bj1) {
                    if (pi <= bi1) acc0 = row[0];
                    if (pi + 8 <= bi1) acc1 = row[8];
                    if (pi + 16 <= bi1) acc2 = row[16];
                    if (pi + 24 <= bi1) acc3 = row[24];
                }
            }
            __syncthreads();
            for (int n = 0; n < total; n++) {
                const int4 b = s_list[n].box;
                const UiRecord r = s_list[n].r;
                const long long x0 = r.x0, y0 = r.y0, x1 = r.x1, y1 = r.y1, x2 = r.x2, y2 = r.y2;
                const float area = (float)surf_edge(x0, y0, x1, y1, x2, y2);
                const unsigned tl = (surf_top_left(x1, y1, x2, y2) ? 1u : 0u) | (surf_top_left(x2, y2, x0, y0) ? 2u : 0u) | (surf_top_left(x0, y0, x1, y1) ? 4u : 0u);
                const long long px = 256ll * pi + 128, py = 256ll * pj + 128;
                // the edge functions at the lane's pixel of tile 0; a tile further right adds 8 pixels' worth of d e / d x = -(by - ay) * 256
                const long long f0 = surf_edge(x1, y1, x2, y2, px, py), f1 = surf_edge(x2, y2, x0, y0, px, py), f2 = surf_edge(x0, y0, x1, y1, px, py);
                const long long s0 = -(y2 - y1) * 2048ll, s1 = -(y0 - y2) * 2048ll, s2 = -(y1 - y0) * 2048ll;
                const bool rowIn = pj >= b.z && pj <= b.w;
                // (a real loop, the pixel picked by selects: unrolled, the four fragment bodies cost scalar registers the kernel does not have)
#pragma unroll 1
                for (int k = 0; k < 4; k++) {
                    const int i = pi + 8 * k;
                    const long long e0 = f0 + s0 * k, e1 = f1 + s1 * k, e2 = f2 + s2 * k;
                    const bool in = rowIn && i >= b.x && i <= b.y && !(e0 < 0 || e1 < 0 || e2 < 0) && !((e0 == 0 && !(tl & 1u)) || (e1 == 0 && !(tl & 2u)) || (e2 == 0 && !(tl & 4u)));
                    if (in) {
                        float4 p = k == 0 ? acc0 : (k == 1 ? acc1 : (k == 2 ? acc2 : acc3));
                        ui_fragment(r, s_unorm, texels, texW, texH, (float)e0 / area, (float)e1 / area, (float)e2 / area, p);
                        if (k == 0) acc0 = p; else if (k == 1) acc1 = p; else if (k == 2) acc2 = p; else acc3 = p;
                        touched |= 1u << k;
                    }
                }
            }
        }
    }
    // (a touched pixel lies inside a box, and boxes are cut to the frame and the band)
    if (touched & 1u) row[0] = acc0;
    if (touched & 2u) row[8] = acc1;
    if (touched & 4u) row[16] = acc2;
    if (touched & 8u) row[24] = acc3;
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int sailor_hip_ui_workspace_bytes(uint32_t numTriangles, int32_t width, int32_t height, size_t* out)
{
    if (!out) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    *out = 0;
    if (!extent_ok(width, height)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    *out = ui_workspace_bytes(numTriangles);
    return SAILOR_HIP_OK;
}

int sailor_hip_ui_draw(SailorHipContext* ctx, const SailorVertexP2UV2C1* dVertices, uint32_t numVertices, const void* dIndices, uint32_t indexBytes, uint32_t numIndices,
                       const SailorUiCommand* commands, const SailorUiCommand* dCommands, uint32_t numCommands, const float* scale, const float* translate,
                       const SailorTextureDesc* texture, void* dWorkspace, size_t workspaceBytes, float* dTarget, int32_t width, int32_t height, const SailorBand* band)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = nullptr;
    unsigned long long triangles = 0;
    if (!extent_ok(width, height)) why = "the extent is not positive (or beyond 32768)";
    else if (!band || sailor_hip_band_is_valid(width, height, band) != 1 || band->fbRowCount < 0) why = "the band is not valid for the frame";
    else if (!scale || !translate || !texture) why = "scale, translate or the texture descriptor is NULL";
    else if (indexBytes != 2u && indexBytes != 4u) why = "the index width is neither 2 nor 4 bytes";
    else if (numCommands > SAILOR_UI_MAX_COMMANDS) why = "more than SAILOR_UI_MAX_COMMANDS commands";
    else if (numCommands && (!commands || !aligned(dCommands, 4))) why = "the command array (host or device) is NULL or not 4-byte aligned";
    else if (texture->flags & SAILOR_TEXTURE_SRGB) why = "the texture is sRGB: the pass samples UNORM";
    else if (texture->texels && (!aligned(texture->texels, 4) || !extent_ok(texture->width, texture->height))) why = "the texture's texels are not 4-byte aligned or its extent is not valid";
    else if (band->fbRowCount > 0 && !aligned(dTarget, 16)) why = "the target is NULL or not 16-byte aligned"; // (a band without rows has no target)
    else if (!aligned(dWorkspace, 16)) why = "the workspace is NULL or not 16-byte aligned";
    for (uint32_t c = 0; !why && c < numCommands; c++) {
        const SailorUiCommand& k = commands[c];
        if ((unsigned long long)k.firstIndex + k.indexCount > numIndices) why = "a command's index range leaves the index buffer";
        else if (k.scissor[0] < 0 || k.scissor[1] < 0 || k.scissor[2] < 0 || k.scissor[3] < 0 || (long long)k.scissor[0] + k.scissor[2] > width ||
                 (long long)k.scissor[1] + k.scissor[3] > height) why = "a command's scissor lies outside the target";
        triangles += k.indexCount / 3u;
    }
    if (!why && triangles > 0xFFFFFFFFull) why = "too many triangles";
    if (!why && triangles && (!aligned(dVertices, 4) || !numVertices)) why = "the vertex buffer is NULL, empty or not 4-byte aligned";
    if (!why && triangles && !aligned(dIndices, indexBytes)) why = "the index buffer is NULL or not aligned to its index width";
    if (!why && workspaceBytes < ui_workspace_bytes((size_t)triangles)) why = "the workspace is smaller than sailor_hip_ui_workspace_bytes answers";
    if (why) return surf_refuse(ctx, "sailor_hip_ui_draw", why);
    if (triangles == 0 || band->fbRowCount == 0) return SAILOR_HIP_OK; // nothing to record
    UiDraw d;
    d.vertices = dVertices; d.indices = dIndices; d.commands = dCommands;
    d.numVertices = numVertices; d.numIndices = numIndices; d.numCommands = numCommands; d.numTriangles = (uint32_t)triangles; d.indexBytes = indexBytes;
    d.scaleX = scale[0]; d.scaleY = scale[1]; d.translateX = translate[0]; d.translateY = translate[1];
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_ui_scan, dim3(1), dim3(256), d, dWorkspace);
    SAILOR_CHECK_LAUNCH(ctx, "k_ui_scan");
    sailor_launch(ctx, k_ui_setup, dim3((unsigned)((triangles + 255) / 256)), dim3(256), d, (int)width, (int)height, (int)band->fbRowBegin, (int)band->fbRowCount, dWorkspace);
    SAILOR_CHECK_LAUNCH(ctx, "k_ui_setup");
    const bool hasTexels = texture->texels && texture->width > 0 && texture->height > 0;
    sailor_launch(ctx, k_ui_blend, dim3((unsigned)((width + UI_BIN - 1) / UI_BIN), (unsigned)((band->fbRowCount + UI_BIN - 1) / UI_BIN)), dim3(256), dCommands, numCommands,
                  (uint32_t)triangles, hasTexels ? texture->texels : nullptr, hasTexels ? (int)texture->width : 0, hasTexels ? (int)texture->height : 0, (int)width, (int)band->fbRowBegin, (int)band->fbRowCount, (const void*)dWorkspace, reinterpret_cast<float4*>(dTarget));
    SAILOR_CHECK_LAUNCH(ctx, "k_ui_blend");
    return SAILOR_HIP_OK;
}

} // extern "C"
