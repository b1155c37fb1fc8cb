"""A restatement of the multisampled surface pass (sailor_amd/csrc/surface_msaa.hip), written from the rules of the Multisampled section of
include/sailor_hip.h: exact integers for the coverage, NumPy float32 for depth, weights and the accumulate.  The set-up, the near-plane cut, the edge function,
the top-left rule and the fragment stage are tests/surface_ref.py's, by import.

Like surface_ref.render it is LITERALLY SEQUENTIAL: primitive after primitive, every SAMPLE tested GreaterOrEqual against a per-sample depth array and written
at once; no keys and no maximum.  The discard of a cutout draw is evaluated once per pixel and primitive with the edge functions of the pixel CENTRE (which may
lie outside the triangle), and removes the primitive from every sample of the pixel.  The sample positions are an argument (host.msaa_sample_positions): the
table is not copied here.

A scene is surface_ref's dict; a draw may carry alpha_cutout (masked_ref's)."""
import numpy as np

import surface_ref as ref
from masked_ref import MaskedTextures
from surface_ref import _edge, _top_left, near_clip, setup, shade_fragments   # noqa: F401  (the restatement is built from these)

f32 = np.float32


def render(scene, positions, rows=None, sample_depth=None):
    """-> dict(store uint64 [n, W, S] (depth bits << 32 | order + 1), inside_count int [n, W, S]: how many primitives cover the sample BEFORE depth and discard,
    stats).  positions: int [S, 2]; rows: the band's framebuffer rows (default: all); sample_depth: float32 [n, W, S] the pass begins from."""
    W, H = scene["W"], scene["H"]
    r0, r1 = rows if rows is not None else (0, H)
    pos = np.asarray(positions, np.int64).reshape(-1, 2)
    S = len(pos)
    V, P = np.asarray(scene["view"], f32).reshape(16), np.asarray(scene["projection"], f32).reshape(16)
    inst, mats = scene["instances"], scene["materials"]
    tex = MaskedTextures(scene["textures"], scene["srgb"])
    depth = np.zeros((H, W, S), f32)
    if sample_depth is not None:
        depth[r0:r1] = np.asarray(sample_depth, f32).reshape(r1 - r0, W, S)
    order_of = np.zeros((H, W, S), np.uint64)
    inside_count = np.zeros((H, W, S), np.int64)
    stats = dict(cut_parts=0, cut_on_edge_pixel=0, tested=0, discarded=0, centre_outside_kept=0, centre_outside_discarded=0, no_centre_primitives=0)
    prim_base = int(scene.get("prim_base", 0))
    with np.errstate(all="ignore"):
        for draw in scene["draws"]:
            verts, indices = np.asarray(draw["vertices"], f32).reshape(-1, 18), np.asarray(draw["indices"], np.uint32).reshape(-1, 3)
            cutout = bool(draw.get("alpha_cutout", False))
            nt, ids = len(indices), draw.get("instance_ids")
            first = int(draw.get("first_instance", 0))
            nd = int(draw["num_drawn"]) if draw.get("num_drawn") is not None else (len(ids) if ids is not None else len(inst) - first)
            for d in range(nd):
                i = int(ids[d]) if ids is not None else first + d
                m = np.asarray(inst["model"][i], f32)
                mi = int(inst["materialInstance"][i])
                material = mats[mi if mi < len(mats) else 0]
                for t in range(nt):
                    idx = [int(q) for q in indices[t]]
                    clip = [ref.glsl_mul(P, *ref.glsl_mul(V, *ref.glsl_mul(m, verts[q][2], verts[q][3], verts[q][4], f32(1)))) for q in idx]
                    for part, (pc, src) in enumerate(near_clip(clip, idx)):
                        order = prim_base + d * 2 * nt + 2 * t + part
                        su = setup(pc, src, W, H, draw.get("cull_back", False))
                        if su is None:
                            continue
                        X, Y, Z, Wc, src = su
                        was_cut = any(s[2] is not None for s in src)
                        # every pixel the bounding box touches; a sample outside the box fails an edge
                        i0, i1 = max(min(X) // 256, 0), min(max(X) // 256, W - 1)
                        j0, j1 = max(min(Y) // 256, r0), min(max(Y) // 256, r1 - 1)
                        if i1 < i0 or j1 < j0:
                            continue
                        ii, jj = np.meshgrid(np.arange(i0, i1 + 1, dtype=np.int64), np.arange(j0, j1 + 1, dtype=np.int64))
                        px, py = 256 * ii[..., None] + pos[:, 0], 256 * jj[..., None] + pos[:, 1]          # [rows, cols, S]
                        e0, e1, e2 = _edge(X[1], Y[1], X[2], Y[2], px, py), _edge(X[2], Y[2], X[0], Y[0], px, py), _edge(X[0], Y[0], X[1], Y[1], px, py)
                        tl0, tl1, tl2 = _top_left(X[1], Y[1], X[2], Y[2]), _top_left(X[2], Y[2], X[0], Y[0]), _top_left(X[0], Y[0], X[1], Y[1])
                        inside = ~((e0 < 0) | (e1 < 0) | (e2 < 0)) & ~(((e0 == 0) & (not tl0)) | ((e1 == 0) & (not tl1)) | ((e2 == 0) & (not tl2)))
                        if not inside.any():
                            continue
                        area = ref._to_f32(_edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]))
                        z = (Z[0] + (Z[1] - Z[0]) * (ref._to_f32(e1) / area)) + (Z[2] - Z[0]) * (ref._to_f32(e2) / area)
                        sub = (slice(j0, j1 + 1), slice(i0, i1 + 1))
                        inside_count[sub] += inside
                        exists = inside & (z > 0) & (z <= 1)
                        passed = exists & (z >= depth[sub])              # GreaterOrEqual, in drawing order, per sample
                        # the pixel centres (the fragment shader's position): may be outside the triangle
                        cx, cy = 256 * ii + 128, 256 * jj + 128
                        c0, c1, c2 = _edge(X[1], Y[1], X[2], Y[2], cx, cy), _edge(X[2], Y[2], X[0], Y[0], cx, cy), _edge(X[0], Y[0], X[1], Y[1], cx, cy)
                        centre_in = ~((c0 < 0) | (c1 < 0) | (c2 < 0)) & ~(((c0 == 0) & (not tl0)) | ((c1 == 0) & (not tl1)) | ((c2 == 0) & (not tl2)))
                        if not centre_in.any():
                            stats["no_centre_primitives"] += 1
                        if was_cut:
                            stats["cut_parts"] += 1
                            stats["cut_on_edge_pixel"] += int((inside.any(-1) & ~inside.all(-1)).sum())
                        some = passed.any(-1)
                        if cutout and some.any():
                            av = []
                            for (I, O, tt) in src:
                                aI = ref.vertex_varyings(verts[I], m)
                                av.append(aI if tt is None else aI + (ref.vertex_varyings(verts[O], m) - aI) * tt)
                            L0, L1, L2 = ref._to_f32(c0[some]) / area, ref._to_f32(c1[some]) / area, ref._to_f32(c2[some]) / area
                            q0, q1, q2 = L0 / Wc[0], L1 / Wc[1], L2 / Wc[2]
                            s = (q0 + q1) + q2
                            b0, b1, b2 = q0 / s, q1 / s, q2 / s
                            alpha = shade_fragments([(av[0][c] * b0 + av[1][c] * b1) + av[2][c] * b2 for c in range(18)], material, tex)[0][..., 3]
                            keep = ~(alpha < f32(0.5))                   # a NaN alpha survives
                            stats["tested"] += int(alpha.size)
                            stats["discarded"] += int((~keep).sum())
                            stats["centre_outside_kept"] += int((keep & ~centre_in[some]).sum())
                            stats["centre_outside_discarded"] += int((~keep & ~centre_in[some]).sum())
                            kept = np.zeros_like(some)
                            kept[some] = keep
                            passed &= kept[..., None]
                        if not passed.any():
                            continue
                        a, b, c = np.nonzero(passed)
                        depth[a + j0, b + i0, c] = z[passed]
                        order_of[a + j0, b + i0, c] = order + 1
            prim_base += nd * 2 * nt
    store = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order_of
    return dict(store=store[r0:r1].copy(), inside_count=inside_count[r0:r1].copy(), stats=stats, next_prim_base=prim_base)


def layers(store, L):
    """rule 7 -> dict(keys uint64 [L, n, W], weights uint8 [L, n, W], uncovered uint8 [n, W], counts int [L], clipped int: the pixels that clip)"""
    store = np.asarray(store, np.uint64)
    n, W, S = store.shape
    assert 1 <= L <= S
    orders, zbits = (store & np.uint64(0xFFFFFFFF)).astype(np.int64), store >> np.uint64(32)
    keys, weights = np.zeros((L, n, W), np.uint64), np.zeros((L, n, W), np.uint8)
    uncovered = (orders == 0).sum(-1).astype(np.uint8)
    clipped = np.zeros((n, W), bool)
    for j in range(n):
        for i in range(W):
            distinct = sorted(set(int(o) for o in orders[j, i] if o))
            for k, o in enumerate(distinct[:L]):
                holders = np.nonzero(orders[j, i] == o)[0]
                keys[k, j, i] = (zbits[j, i, holders[0]] << np.uint64(32)) | np.uint64(o)
                weights[k, j, i] = len(holders)
            if len(distinct) > L:
                weights[L - 1, j, i] += int((orders[j, i] > distinct[L - 1]).sum())
                clipped[j, i] = True
    return dict(keys=keys, weights=weights, uncovered=uncovered, counts=(weights > 0).sum((1, 2)), clipped=int(clipped.sum()))


def accumulate(target, colour, weight, uncovered, S, k):
    """rule 9 for layer k, in place on a copy: target, colour float32 [n, W, 4]; weight, uncovered uint8 [n, W].  Every product and sum rounded on its own;
    a term of weight 0 is omitted; w_0 == S stores the colour's bits."""
    out = np.array(target, f32)
    colour = np.asarray(colour, f32)
    w, u = np.asarray(weight).astype(np.int64), np.asarray(uncovered).astype(np.int64)
    fw, fu = (w.astype(f32) / f32(S))[..., None], (u.astype(f32) / f32(S))[..., None]
    with np.errstate(all="ignore"):
        term = (fw * colour).astype(f32)
        if k == 0:
            whole, part = w == S, (w > 0) & (w < S)
            out.view(np.uint32)[whole] = colour.view(np.uint32)[whole]
            alone, over = part & (u == 0), part & (u > 0)
            out[alone] = term[alone]
            out[over] = ((fu * np.asarray(target, f32)).astype(f32) + term)[over]
        else:
            has = w > 0
            out[has] = (np.asarray(target, f32) + term)[has]
    return out


def depth_out(store):
    """rule 10 -> (the sample depths float32 [n, W, S], their AVERAGE float32 [n, W]: (((z_0 + z_1) + ...) + z_(S-1)) * (1 / S))"""
    z = (np.asarray(store, np.uint64) >> np.uint64(32)).astype(np.uint32).view(f32)
    S = z.shape[-1]
    total = z[..., 0].copy()
    with np.errstate(all="ignore"):
        for s in range(1, S):
            total = total + z[..., s]
        return z, total * (f32(1) / f32(S))
