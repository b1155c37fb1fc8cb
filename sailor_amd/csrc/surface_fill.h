// The fill of a set-up triangle, once, for every draw kernel of the surface pass and of the particles (k_surface_visibility, surf_visibility_masked's four
// kernels, k_particles_raster's two): small triangles are filled by their lane, stepping the edge functions texel by texel in exact integers as
// k_raster_depth does; large ones are handed round the wave -- the 64 x 64 superblocks of the box one after the other, of each the 8 x 8 blocks one per
// lane, the blocks an edge does not rule out one lane per texel.  frag(i, j, z, tag, payload, e0, e1, e2, area) is called for every fragment of the box
// that passes the edge functions, the top-left rule and 0 < z <= 1, with the tag and the payload of the lane that set the triangle up: what that lane
// knows of its triangle beyond the geometry.  bcast(payload, src) carries it to the wave, once per large triangle, never per fragment; a kernel with
// nothing to carry passes SurfNoPayload and SurfNoBcast.  Every lane of the wave has to arrive (the large path ballots).  slice / slices are the
// gridDim.y slices (surface.hip): slice 0 fills the small ones, and of a large triangle's superblocks slice y takes those whose running number is y
// modulo the slices.  tests/surface_ref.py restates the walk sequentially, and the tests hold every caller to it bit for bit.
#pragma once
#include "surface_common.h"

// keeps a (wave-uniform or boolean) value in a vector register: the scalar file of the masked draw kernels is full (two matrices, the draw, the loops' masks)
#define SURF_KEEP_VECTOR(x) asm volatile("" : "+v"(x))

struct SurfNoPayload {};
struct SurfNoBcast { __device__ __forceinline__ SurfNoPayload operator()(const SurfNoPayload&, int) const { return SurfNoPayload(); } };

// the three top-left flags as bits of one vector register, for every caller: as three booleans they are three scalar pairs through the loops, which the
// masked kernels do not have; the opaque and the particle kernels keep their registers and their times either way (the A/B of the surface pass)
__device__ __forceinline__ int surf_top_left_bits(const SurfTri& t)
{
    int tl = (surf_top_left(t.x1, t.y1, t.x2, t.y2) ? 1 : 0) | (surf_top_left(t.x2, t.y2, t.x0, t.y0) ? 2 : 0) | (surf_top_left(t.x0, t.y0, t.x1, t.y1) ? 4 : 0);
    SURF_KEEP_VECTOR(tl);
    return tl;
}
// an edge value of 0 counts only on a top or left edge.  (Called behind the test that no edge value is negative, and kept apart from it: the compiler then
// converts e1 and e2 for the depth as unsigned, which is shorter.)
__device__ __forceinline__ bool surf_on_excluded_edge(long long e0, long long e1, long long e2, int tl)
{
    return (e0 == 0 && !(tl & 1)) || (e1 == 0 && !(tl & 2)) || (e2 == 0 && !(tl & 4));
}
__device__ __forceinline__ float surf_depth(const SurfTri& t, long long e1, long long e2, float area)
{
    return (t.z0 + (t.z1 - t.z0) * ((float)e1 / area)) + (t.z2 - t.z0) * ((float)e2 / area);
}

template <typename P, typename B, typename F>
__device__ __forceinline__ void surf_fill(const SurfTri& t, unsigned int tag, const P& payload, B bcast, unsigned int slice, unsigned int slices, int lane, F frag)
{
    const bool small = t.valid && (long long)(t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) <= SURF_SMALL_BOX;
    if (small && slice == 0) {
        const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
        const int tl = surf_top_left_bits(t);
        const long long px0 = 256ll * t.i0 + 128, py0 = 256ll * t.j0 + 128;
        long long r0 = surf_edge(t.x1, t.y1, t.x2, t.y2, px0, py0), r1 = surf_edge(t.x2, t.y2, t.x0, t.y0, px0, py0), r2 = surf_edge(t.x0, t.y0, t.x1, t.y1, px0, py0);
        const long long dx0 = -256ll * (t.y2 - t.y1), dx1 = -256ll * (t.y0 - t.y2), dx2 = -256ll * (t.y1 - t.y0);
        const long long dy0 = 256ll * (t.x2 - t.x1), dy1 = 256ll * (t.x0 - t.x2), dy2 = 256ll * (t.x1 - t.x0);
        for (int j = t.j0; j <= t.j1; j++, r0 += dy0, r1 += dy1, r2 += dy2) {
            long long e0 = r0, e1 = r1, e2 = r2;
            for (int i = t.i0; i <= t.i1; i++, e0 += dx0, e1 += dx1, e2 += dx2) {
                if (e0 < 0 || e1 < 0 || e2 < 0) continue;
                if (surf_on_excluded_edge(e0, e1, e2, tl)) continue;
                const float z = surf_depth(t, e1, e2, area);
                if (z > 0.0f && z <= 1.0f) frag(i, j, z, tag, payload, e0, e1, e2, area);
            }
        }
    }
    // the large ones: the whole wave on one triangle at a time; the payload travels with the geometry
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
        const auto bPayload = bcast(payload, src);
        const float area = (float)surf_edge(b.x0, b.y0, b.x1, b.y1, b.x2, b.y2);
        const int tl = surf_top_left_bits(b);
        // a block wholly outside an edge is dropped (an edge function is affine, so its largest value over the block sits at a corner texel)
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
                        const bool in = !(e0 < 0 || e1 < 0 || e2 < 0) && !surf_on_excluded_edge(e0, e1, e2, tl);
                        if (in) {
                            const float z = surf_depth(b, e1, e2, area);
                            if (z > 0.0f && z <= 1.0f) frag(i, j, z, bTag, bPayload, e0, e1, e2, area);
                        }
                    }
                }
            }
    }
}
