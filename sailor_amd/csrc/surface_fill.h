// The fill of a set-up triangle as k_surface_visibility does it (surface.hip has the notes), with what happens to a fragment left to the caller: small
// triangles are filled by their lane, large ones are handed round the wave -- the 8 x 8 blocks of a 64 x 64 superblock one per lane, the blocks an edge does
// not rule out one lane per texel.  frag(i, j, z, tag) is called for every fragment of the box that passes the edge functions, the top-left rule and
// 0 < z <= 1, with the tag of the lane that set the triangle up.  Every lane of the wave has to arrive (the large path ballots); slice / slices are
// k_surface_visibility's gridDim.y slices.  For particles.hip, whose two passes differ in the key alone; the surface kernels keep their own spelled-out
// copies (their register allocation is tuned around them).  AUTHORITATIVE is k_surface_visibility in surface.hip: this file and surf_visibility_masked
// (surface_masked_body.h) restate its walk and must change with it; the tests hold all three to the one sequential restatement, tests/surface_ref.py.
#pragma once
#include "surface_common.h"

template <typename F>
__device__ __forceinline__ void surf_fill(const SurfTri& t, unsigned int tag, unsigned int slice, unsigned int slices, int lane, F frag)
{
    const bool small = t.valid && (long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) <= SURF_SMALL_BOX;
    if (small && slice == 0) {
        const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
        const bool tl0 = surf_top_left(t.x1, t.y1, t.x2, t.y2), tl1 = surf_top_left(t.x2, t.y2, t.x0, t.y0), tl2 = surf_top_left(t.x0, t.y0, t.x1, t.y1);
        const long long px0 = 256ll * t.i0 + 128, py0 = 256ll * t.j0 + 128;
        long long r0 = surf_edge(t.x1, t.y1, t.x2, t.y2, px0, py0), r1 = surf_edge(t.x2, t.y2, t.x0, t.y0, px0, py0), r2 = surf_edge(t.x0, t.y0, t.x1, t.y1, px0, py0);
        const long long dx0 = -256ll * (t.y2 - t.y1), dx1 = -256ll * (t.y0 - t.y2), dx2 = -256ll * (t.y1 - t.y0);
        const long long dy0 = 256ll * (t.x2 - t.x1), dy1 = 256ll * (t.x0 - t.x2), dy2 = 256ll * (t.x1 - t.x0);
        for (int j = t.j0; j <= t.j1; j++, r0 += dy0, r1 += dy1, r2 += dy2) {
            long long e0 = r0, e1 = r1, e2 = r2;
            for (int i = t.i0; i <= t.i1; i++, e0 += dx0, e1 += dx1, e2 += dx2) {
                if (e0 < 0 || e1 < 0 || e2 < 0) continue;
                if ((e0 == 0 && !tl0) || (e1 == 0 && !tl1) || (e2 == 0 && !tl2)) continue;
                const float z = (t.z0 + (t.z1 - t.z0) * ((float)e1 / area)) + (t.z2 - t.z0) * ((float)e2 / area);
                if (z > 0.0f && z <= 1.0f) frag(i, j, z, tag);
            }
        }
    }
    unsigned long long todo = __ballot(t.valid && !small);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        SurfTri b;
        b.x0 = surf_bcast64(t.x0, src); b.y0 = surf_bcast64(t.y0, src); b.x1 = surf_bcast64(t.x1, src); b.y1 = surf_bcast64(t.y1, src);
        b.x2 = surf_bcast64(t.x2, src); b.y2 = surf_bcast64(t.y2, src);
        b.z0 = __shfl(t.z0, src, 64); b.z1 = __shfl(t.z1, src, 64); b.z2 = __shfl(t.z2, src, 64);
        b.i0 = __shfl(t.i0, src, 64); b.i1 = __shfl(t.i1, src, 64); b.j0 = __shfl(t.j0, src, 64); b.j1 = __shfl(t.j1, src, 64);
        const unsigned int bTag = (unsigned int)__shfl((int)tag, src, 64);
        const float area = (float)surf_edge(b.x0, b.y0, b.x1, b.y1, b.x2, b.y2);
        const bool tl0 = surf_top_left(b.x1, b.y1, b.x2, b.y2), tl1 = surf_top_left(b.x2, b.y2, b.x0, b.y0), tl2 = surf_top_left(b.x0, b.y0, b.x1, b.y1);
        unsigned int number = 0;
        for (int sj = b.j0 >> 6; sj <= (b.j1 >> 6); sj++)
            for (int si = b.i0 >> 6; si <= (b.i1 >> 6); si++) {
                if (number++ % slices != slice) continue;
                const int bi = si * 8 + (lane & 7), bj = sj * 8 + (lane >> 3);
                bool alive = bi >= (b.i0 >> 3) && bi <= (b.i1 >> 3) && bj >= (b.j0 >> 3) && bj <= (b.j1 >> 3);
                if (alive) {
                    long long m0 = -0x7FFFFFFFFFFFFFFFll, m1 = m0, m2 = m0;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const long long px = 256ll * (bi * 8 + ((c & 1) ? 7 : 0)) + 128, py = 256ll * (bj * 8 + ((c & 2) ? 7 : 0)) + 128;
                        m0 = max(m0, surf_edge(b.x1, b.y1, b.x2, b.y2, px, py)); m1 = max(m1, surf_edge(b.x2, b.y2, b.x0, b.y0, px, py));
                        m2 = max(m2, surf_edge(b.x0, b.y0, b.x1, b.y1, px, py));
                    }
                    alive = m0 >= 0 && m1 >= 0 && m2 >= 0;
                }
                unsigned long long live = __ballot(alive);
                while (live) { // the surviving blocks, one lane per texel
                    const int s2 = __builtin_ctzll(live);
                    live &= live - 1ull;
                    const int i = (si * 8 + (s2 & 7)) * 8 + (lane & 7), j = (sj * 8 + (s2 >> 3)) * 8 + (lane >> 3);
                    if (i >= b.i0 && i <= b.i1 && j >= b.j0 && j <= b.j1) {
                        const long long px = 256ll * i + 128, py = 256ll * j + 128;
                        const long long e0 = surf_edge(b.x1, b.y1, b.x2, b.y2, px, py), e1 = surf_edge(b.x2, b.y2, b.x0, b.y0, px, py),
                                        e2 = surf_edge(b.x0, b.y0, b.x1, b.y1, px, py);
                        const bool in = !(e0 < 0 || e1 < 0 || e2 < 0) && !((e0 == 0 && !tl0) || (e1 == 0 && !tl1) || (e2 == 0 && !tl2));
                        if (in) {
                            const float z = (b.z0 + (b.z1 - b.z0) * ((float)e1 / area)) + (b.z2 - b.z0) * ((float)e2 / area);
                            if (z > 0.0f && z <= 1.0f) frag(i, j, z, bTag);
                        }
                    }
                }
            }
    }
}
