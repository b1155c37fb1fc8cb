// The fill of a set-up triangle for the multisampled pass (surface_msaa.hip): surf_fill's walk (surface_fill.h) over PIXELS, not centres.  The three edge
// functions are stepped at the pixel centres as there, in exact integers; a sample's values are the centre's plus an offset that is affine in the sample's
// position, gx[k] * (sx - 128) + gy[k] * (sy - 128), with gx, gy the edge's steps per 1/256 pixel: six 32-bit words a triangle (a snapped coordinate is below
// 1e9 in magnitude, so a difference of two fits).  The sample table travels as ONE 64-bit word -- byte s = (sy / 16) << 4 | (sx / 16): every standard
// position is a multiple of 16 inside 16 .. 240 -- so an offset costs two 32 x 32 -> 64 multiply-adds and no table in memory or in registers.
//
// From the largest and the smallest offset of each edge over the S samples (hi, lo; once per triangle) a pixel is
//   rejected      when some centre value + hi is negative: no sample of it can be inside that edge;
//   taken `full`  when every centre value + lo is positive: every sample is strictly inside all three edges, no per-sample edge test, no top-left rule;
// and handed to pix(i, j, tri, edges, tl, full, tag, payload, e0, e1, e2, area) otherwise, with the CENTRE's edge values (which may be negative: the centre
// need not be covered).  The large path bounds a block by its pixel squares: the largest centre value over the block's corner pixels plus hi.
// The box is the set-up's PIXEL_BOX (every pixel the bounding box touches), a superset of the pixels that hold a sample inside the bounding box; the
// others fall to the reject above.  tests/msaa_ref.py restates the coverage sample by sample, and the tests hold the kernels to it bit for bit.
#pragma once
#include "surface_fill.h"

struct SurfMsaaEdges { int gx[3], gy[3]; long long hi[3], lo[3]; };

__device__ __forceinline__ int surf_msaa_dx(unsigned long long pattern, int s) { return (int)((unsigned int)(pattern >> (8 * s)) & 15u) * 16 - 128; }
__device__ __forceinline__ int surf_msaa_dy(unsigned long long pattern, int s) { return (int)((unsigned int)(pattern >> (8 * s + 4)) & 15u) * 16 - 128; }
// edge function k of the sample at (mx, my) from the pixel centre
__device__ __forceinline__ long long surf_msaa_at(const SurfMsaaEdges& m, int k, long long e, int mx, int my)
{
    return e + ((long long)m.gx[k] * mx + (long long)m.gy[k] * my);
}

__device__ __forceinline__ SurfMsaaEdges surf_msaa_edges(const SurfTri& t, int S, unsigned long long pattern)
{
    SurfMsaaEdges m;
    m.gx[0] = (int)-(t.y2 - t.y1); m.gx[1] = (int)-(t.y0 - t.y2); m.gx[2] = (int)-(t.y1 - t.y0);
    m.gy[0] = (int)(t.x2 - t.x1); m.gy[1] = (int)(t.x0 - t.x2); m.gy[2] = (int)(t.x1 - t.x0);
#pragma unroll
    for (int k = 0; k < 3; k++) { m.hi[k] = -0x7FFFFFFFFFFFFFFFll; m.lo[k] = 0x7FFFFFFFFFFFFFFFll; }
#pragma unroll 1
    for (int s = 0; s < S; s++) {
        const int mx = surf_msaa_dx(pattern, s), my = surf_msaa_dy(pattern, s);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long long o = surf_msaa_at(m, k, 0, mx, my);
            m.hi[k] = max(m.hi[k], o); m.lo[k] = min(m.lo[k], o);
        }
    }
    return m;
}

template <typename P, typename B, typename F>
__device__ __forceinline__ void surf_fill_msaa(const SurfTri& t, unsigned int tag, const P& payload, B bcast, unsigned int slice, unsigned int slices, int lane, int S,
                                               unsigned long long pattern, F pix)
{
    const bool small = t.valid && (long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) <= SURF_SMALL_BOX;
    if (small && slice == 0) {
        const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
        const int tl = surf_top_left_bits(t);
        const SurfMsaaEdges m = surf_msaa_edges(t, S, pattern);
        const long long px0 = 256ll * t.i0 + 128, py0 = 256ll * t.j0 + 128;
        long long r0 = surf_edge(t.x1, t.y1, t.x2, t.y2, px0, py0), r1 = surf_edge(t.x2, t.y2, t.x0, t.y0, px0, py0), r2 = surf_edge(t.x0, t.y0, t.x1, t.y1, px0, py0);
        const long long dx0 = 256ll * m.gx[0], dx1 = 256ll * m.gx[1], dx2 = 256ll * m.gx[2];
        const long long dy0 = 256ll * m.gy[0], dy1 = 256ll * m.gy[1], dy2 = 256ll * m.gy[2];
        for (int j = t.j0; j <= t.j1; j++, r0 += dy0, r1 += dy1, r2 += dy2) {
            long long e0 = r0, e1 = r1, e2 = r2;
            for (int i = t.i0; i <= t.i1; i++, e0 += dx0, e1 += dx1, e2 += dx2) {
                if (e0 + m.hi[0] < 0 || e1 + m.hi[1] < 0 || e2 + m.hi[2] < 0) continue;
                const bool full = e0 + m.lo[0] > 0 && e1 + m.lo[1] > 0 && e2 + m.lo[2] > 0;
                pix(i, j, t, m, tl, full, tag, payload, e0, e1, e2, area);
            }
        }
    }
    // the large ones: the whole wave on one triangle at a time, as surf_fill
    unsigned long long todo = __ballot(t.valid && !small);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        SurfTri b;
        b.x0 = surf_bcast64(t.x0, src); b.y0 = surf_bcast64(t.y0, src); b.x1 = surf_bcast64(t.x1, src); b.y1 = surf_bcast64(t.y1, src);
        b.x2 = surf_bcast64(t.x2, src); b.y2 = surf_bcast64(t.y2, src);
        b.z0 = __shfl(t.z0, src, 64); b.z1 = __shfl(t.z1, src, 64); b.z2 = __shfl(t.z2, src, 64);
        b.i0 = __shfl(t.i0, src, 64); b.i1 = __shfl(t.i1, src, 64); b.j0 = __shfl(t.j0, src, 64); b.j1 = __shfl(t.j1, src, 64);
        b.valid = true;
        const unsigned int bTag = (unsigned int)__shfl((int)tag, src, 64);
        const auto bPayload = bcast(payload, src);
        const float area = (float)surf_edge(b.x0, b.y0, b.x1, b.y1, b.x2, b.y2);
        const int tl = surf_top_left_bits(b);
        const SurfMsaaEdges m = surf_msaa_edges(b, S, pattern);
        unsigned int number = 0;
        for (int sj = b.j0 >> 6; sj <= (b.j1 >> 6); sj++)
            for (int si = b.i0 >> 6; si <= (b.i1 >> 6); si++) {
                if (number++ % slices != slice) continue;
                const int bi = si * 8 + (lane & 7), bj = sj * 8 + (lane >> 3);
                bool alive = bi >= (b.i0 >> 3) && bi <= (b.i1 >> 3) && bj >= (b.j0 >> 3) && bj <= (b.j1 >> 3);
                if (alive) {
                    // an edge function is affine: its largest value over the block's pixel SQUARES is below the largest centre value of the corner pixels + hi
                    long long m0 = -0x7FFFFFFFFFFFFFFFll, m1 = m0, m2 = m0;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const long long px = 256ll * (bi * 8 + ((c & 1) ? 7 : 0)) + 128, py = 256ll * (bj * 8 + ((c & 2) ? 7 : 0)) + 128;
                        m0 = max(m0, surf_edge(b.x1, b.y1, b.x2, b.y2, px, py)); m1 = max(m1, surf_edge(b.x2, b.y2, b.x0, b.y0, px, py));
                        m2 = max(m2, surf_edge(b.x0, b.y0, b.x1, b.y1, px, py));
                    }
                    alive = m0 + m.hi[0] >= 0 && m1 + m.hi[1] >= 0 && m2 + m.hi[2] >= 0;
                }
                unsigned long long live = __ballot(alive);
                while (live) { // the surviving blocks, one lane per pixel
                    const int s2 = __builtin_ctzll(live);
                    live &= live - 1ull;
                    const int i = (si * 8 + (s2 & 7)) * 8 + (lane & 7), j = (sj * 8 + (s2 >> 3)) * 8 + (lane >> 3);
                    if (i >= b.i0 && i <= b.i1 && j >= b.j0 && j <= b.j1) {
                        const long long px = 256ll * i + 128, py = 256ll * j + 128;
                        const long long e0 = surf_edge(b.x1, b.y1, b.x2, b.y2, px, py), e1 = surf_edge(b.x2, b.y2, b.x0, b.y0, px, py),
                                        e2 = surf_edge(b.x0, b.y0, b.x1, b.y1, px, py);
                        if (!(e0 + m.hi[0] < 0 || e1 + m.hi[1] < 0 || e2 + m.hi[2] < 0)) {
                            const bool full = e0 + m.lo[0] > 0 && e1 + m.lo[1] > 0 && e2 + m.lo[2] > 0;
                            pix(i, j, b, m, tl, full, bTag, bPayload, e0, e1, e2, area);
                        }
                    }
                }
            }
    }
}
