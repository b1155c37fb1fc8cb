"""A float32 NumPy restatement of the Masked render queue (sailor_amd/csrc/surface_masked.hip): tests/surface_ref.py's sequential surface pass with
Standard.shader:403-408 `if (material.albedo.a < 0.5) discard;` for the draws that carry alpha_cutout=True, written from the rules pinned in
include/sailor_hip.h.

Like surface_ref.render it is LITERALLY SEQUENTIAL -- draw after draw, a >= test against a depth array, no keys and no maximum -- and a discarded fragment is
dropped BEFORE the depth test's write: it writes no depth, no planes, no order, and takes no part in ties.  The alpha that is tested is not a second
formula: it is P0.w of surface_ref.shade_fragments on the interpolated varyings, (material.albedo[3] * tA.w) * a[8].

Next to the result it reports a float64 twin of every tested alpha (alpha64: the same formula over the same float32 inputs and the same exact edge
functions, every operation in double), the screen-linear MUTANT (perspective=False: b_k = l_k), and counts: fragments tested, discarded, NaN alphas, alphas
exactly 0.5, fragments discarded at a depth tie.

A scene is surface_ref's dict; a draw may carry alpha_cutout (default False).  A texture of shape (0, 0, 4) is a descriptor without texels: it samples 0."""
import numpy as np

import surface_ref as ref
from surface_ref import Textures, near_clip, setup, shade_fragments, vertex_varyings   # noqa: F401  (the restatement is built from these)

f32, f64 = np.float32, np.float64


class MaskedTextures(Textures):
    """surface_ref.Textures with descriptors without texels (shape (0, 0, 4)): they sample 0, as the header says"""

    def sample(self, index, u, v):
        at = index if index < len(self.images) else 0
        if self.images[at].shape[0] == 0 or self.images[at].shape[1] == 0:
            if index >= len(self.images):
                self.beyond += 1
            return np.zeros(np.shape(u) + (4,), f32)
        return super().sample(index, u, v)


def _alpha64(av, l64, wc, material, images, perspective):
    """the float64 twin: av = the three vertices' float32 varyings, l64 = the three l_k in double [n], wc = the three clip w"""
    if perspective:
        q = [l64[k] / f64(wc[k]) for k in range(3)]
        s = (q[0] + q[1]) + q[2]
        b = [q[k] / s for k in range(3)]
    else:
        b = l64
    a = {c: (f64(av[0][c]) * b[0] + f64(av[1][c]) * b[1]) + f64(av[2][c]) * b[2] for c in (0, 1, 8)}
    index = int(material["albedoSampler"])
    img = images[index if index < len(images) else 0]
    h, w = img.shape[:2]
    if h == 0 or w == 0:
        t = np.zeros_like(a[0])
    else:
        def tap(n, c):
            x = c * n - 0.5
            fx = np.floor(x)
            i0 = ref.sat_int(fx) % n
            return i0, np.where(i0 + 1 == n, 0, i0 + 1), x - fx
        x0, x1, ax = tap(w, a[0])
        y0, y1, ay = tap(h, a[1])
        al = img[..., 3].astype(f64) / 255.0
        top = al[y0, x0] * (1 - ax) + al[y0, x1] * ax
        bot = al[y1, x0] * (1 - ax) + al[y1, x1] * ax
        t = top * (1 - ay) + bot * ay
    return (f64(material["albedo"][3]) * t) * a[8]


def render(scene, prepass=None, rows=None, perspective=True):
    """surface_ref.render's result and stats, plus: cutout bool [n, W] (the pixel's owner is a fragment of a cutout draw), alpha32 / alpha64 (every tested
    fragment's alpha, in the order tested), and in stats: tested, discarded, nan_alpha, exactly_half, discarded_at_tie."""
    W, H = scene["W"], scene["H"]
    r0, r1 = rows if rows is not None else (0, H)
    V, P = np.asarray(scene["view"], f32).reshape(16), np.asarray(scene["projection"], f32).reshape(16)
    inst, mats = scene["instances"], scene["materials"]
    tex = MaskedTextures(scene["textures"], scene["srgb"])
    depth = np.zeros((H, W), f32) if prepass is None else np.array(prepass, f32).reshape(H, W).copy()
    covered = np.zeros((H, W), bool)
    cutout_owner = np.zeros((H, W), bool)
    order_of = np.zeros((H, W), np.uint64)
    planes = np.empty((3, H, W, 4), f32)
    for k in range(3):
        planes[k] = ref.UNCOVERED[k]
    stats = dict(cut_one=0, cut_two=0, ties=0, fragments=0, overwritten=0, culled=0, degenerate=0, clipped_away=0, large=0, materials=set(), swapped=0,
                 tested=0, discarded=0, nan_alpha=0, exactly_half=0, discarded_at_tie=0)
    alpha32, alpha64 = [], []
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
                    parts = near_clip(clip, idx)
                    if not parts:
                        stats["clipped_away"] += 1
                    if len(parts) == 2:
                        stats["cut_two"] += 1
                    elif len(parts) == 1 and any(s[2] is not None for s in parts[0][1]):
                        stats["cut_one"] += 1
                    for part, (pc, src) in enumerate(parts):
                        order = prim_base + d * 2 * nt + 2 * t + part
                        su = setup(pc, src, W, H, draw.get("cull_back", False))
                        if su is None:
                            stats["degenerate"] += 1
                            continue
                        X, Y, Z, Wc, src = su
                        i0, i1 = max((min(X) - 128 + 255) // 256, 0), min((max(X) - 128) // 256, W - 1)
                        j0, j1 = max((min(Y) - 128 + 255) // 256, r0), min((max(Y) - 128) // 256, r1 - 1)
                        if i1 < i0 or j1 < j0:
                            continue
                        if (i1 - i0 + 1) * (j1 - j0 + 1) > 64:
                            stats["large"] += 1
                        px, py = np.meshgrid(256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128, 256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)
                        e0, e1, e2 = ref._edge(X[1], Y[1], X[2], Y[2], px, py), ref._edge(X[2], Y[2], X[0], Y[0], px, py), ref._edge(X[0], Y[0], X[1], Y[1], px, py)
                        tl0, tl1, tl2 = ref._top_left(X[1], Y[1], X[2], Y[2]), ref._top_left(X[2], Y[2], X[0], Y[0]), ref._top_left(X[0], Y[0], X[1], Y[1])
                        inside = ~((e0 < 0) | (e1 < 0) | (e2 < 0)) & ~(((e0 == 0) & (not tl0)) | ((e1 == 0) & (not tl1)) | ((e2 == 0) & (not tl2)))
                        area_i = ref._edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
                        area = ref._to_f32(area_i)
                        l0, l1, l2 = ref._to_f32(e0) / area, ref._to_f32(e1) / area, ref._to_f32(e2) / area
                        z = (Z[0] + (Z[1] - Z[0]) * l1) + (Z[2] - Z[0]) * l2
                        sub = (slice(j0, j1 + 1), slice(i0, i1 + 1))
                        exists = inside & (z > 0) & (z <= 1)
                        passed = exists & (z >= depth[sub])            # GreaterOrEqual, in drawing order
                        if not passed.any():
                            continue
                        av = []
                        for (I, O, tt) in src:
                            aI = vertex_varyings(verts[I], m)
                            av.append(aI if tt is None else aI + (vertex_varyings(verts[O], m) - aI) * tt)

                        def fragments(mask):
                            L0, L1, L2 = l0[mask], l1[mask], l2[mask]
                            if perspective:
                                q0, q1, q2 = L0 / Wc[0], L1 / Wc[1], L2 / Wc[2]
                                s = (q0 + q1) + q2
                                b0, b1, b2 = q0 / s, q1 / s, q2 / s
                            else:
                                b0, b1, b2 = L0, L1, L2
                            return shade_fragments([(av[0][c] * b0 + av[1][c] * b1) + av[2][c] * b2 for c in range(18)], material, tex)
                        if cutout:
                            # the discard, before anything of the fragment is written: alpha = P0.w of the very shading that would be written
                            beyond, taps = tex.beyond, dict(tex.taps)
                            alpha = fragments(passed)[0][..., 3]
                            tex.beyond, tex.taps = beyond, taps           # (the survivors are shaded -- and counted -- below)
                            keep = ~(alpha < f32(0.5))                    # a NaN alpha survives
                            stats["tested"] += int(alpha.size)
                            stats["discarded"] += int((~keep).sum())
                            stats["nan_alpha"] += int(np.isnan(alpha).sum())
                            stats["exactly_half"] += int((alpha == f32(0.5)).sum())
                            stats["discarded_at_tie"] += int((~keep & (z[passed] == depth[sub][passed])).sum())
                            alpha32.append(alpha)
                            e = [q[passed].astype(f64) / f64(area_i) for q in (e0, e1, e2)]
                            alpha64.append(_alpha64(av, e, Wc, material, tex.images, perspective))
                            survivors = np.zeros_like(passed)
                            survivors[passed] = keep
                            passed = survivors
                            if not passed.any():
                                continue
                        stats["fragments"] += int(passed.sum())
                        stats["ties"] += int((passed & (z == depth[sub])).sum())
                        stats["overwritten"] += int((passed & covered[sub]).sum())
                        stats["materials"].add(mi)
                        p0, p1, p2 = fragments(passed)
                        jj, ii = np.nonzero(passed)
                        jj, ii = jj + j0, ii + i0
                        planes[0, jj, ii], planes[1, jj, ii], planes[2, jj, ii] = p0, p1, p2
                        depth[jj, ii] = z[passed]
                        covered[jj, ii] = True
                        cutout_owner[jj, ii] = cutout
                        order_of[jj, ii] = order + 1
            prim_base += nd * 2 * nt
    stats["beyond_table"], stats["taps"] = tex.beyond, tex.taps
    keys = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order_of
    cat = lambda a, t: np.concatenate([np.ravel(x) for x in a]).astype(t) if a else np.zeros(0, t)
    return dict(planes=planes[:, r0:r1].copy(), depth=depth[r0:r1].copy(), covered=covered[r0:r1].copy(), keys=keys[r0:r1].copy(), stats=stats,
                next_prim_base=prim_base, cutout=cutout_owner[r0:r1].copy(), alpha32=cat(alpha32, f32), alpha64=cat(alpha64, f64))


def masked_prepass_depth(scene, opaque_depth):
    """DepthPrepass `Tag: Masked` over the scene's cutout draws, begun from the Opaque prepass's depth: the restatement's depth (a discarded fragment writes none)"""
    s = dict(scene)
    s["draws"] = [d for d in scene["draws"] if d.get("alpha_cutout", False)]
    return render(s, prepass=opaque_depth)["depth"]
