"""A float32 NumPy restatement of glTF materials in the surface pass (sailor_amd/csrc/surface_gltf.hip): tests/masked_ref.py's sequential pass in which a draw
may carry gltf=True -- Content/Shaders/Standard_glTF.shader where it differs from Standard.shader, written from the rules pinned in include/sailor_hip.h
(the glTF section): the tangent basis under transpose(inverse(mat3(model))) in glm's form, the material slot read as the glTF record, the orm / occlusion /
emissive fetches, normalScale, and `discard` against the material's alphaCutoff.

Like surface_ref.render it is LITERALLY SEQUENTIAL -- draw after draw, a >= test against a depth array, no keys and no maximum; a discarded fragment is dropped
before anything of it is written.  A draw without gltf goes through surface_ref's own vertex_varyings and shade_fragments, untouched.

A scene is surface_ref's dict; a draw may carry alpha_cutout and gltf (default False); the scene may carry ao_in (float32 [H, W]: g_AO at the pixel, None = 1).
`materials` stays ONE array of 80-byte slots (sailor_amd._lib.MATERIAL_DTYPE records); a glTF draw reads a slot through _lib.GLTF_MATERIAL_DTYPE."""
import numpy as np

import surface_ref as ref
from masked_ref import MaskedTextures
from sailor_amd import _lib
from surface_ref import near_clip, setup

f32, f64 = np.float32, np.float64
GLTF = np.dtype(_lib.GLTF_MATERIAL_DTYPE)
NO_EMISSIVE = np.array([0, 0, 0, 1], f32)


def normal_matrix(m):
    """transpose(inverse(mat3(model))) in glm's 3 x 3 form, one float32 rounding per written operation -> N[c][r] as 9 floats, column after column"""
    m = np.asarray(m, f32)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
    c00, c01, c02 = m11 * m22 - m21 * m12, m01 * m22 - m21 * m02, m01 * m12 - m11 * m02
    det = (m00 * c00 - m10 * c01) + m20 * c02
    one_over_det = f32(1) / det
    inv = {(0, 0): c00 * one_over_det, (1, 0): -(m10 * m22 - m20 * m12) * one_over_det, (2, 0): (m10 * m21 - m20 * m11) * one_over_det,
           (0, 1): -c01 * one_over_det, (1, 1): (m00 * m22 - m20 * m02) * one_over_det, (2, 1): -(m00 * m21 - m20 * m01) * one_over_det,
           (0, 2): c02 * one_over_det, (1, 2): -(m00 * m12 - m10 * m02) * one_over_det, (2, 2): (m00 * m11 - m10 * m01) * one_over_det}   # inv[(col, row)]
    return np.array([inv[(r, c)] for c in range(3) for r in range(3)], f32)   # N[c][r] = I[r][c]


def vertex_varyings(v, m, standard_basis=False):
    """the 18 varyings of Standard_glTF.shader:130-141: Standard.shader's, with tangentBasis = N * mat3(inTangent, inBitangent, inNormal).
    standard_basis=True is the MUTANT that keeps Standard.shader's mat3(model)"""
    out = ref.vertex_varyings(v, m)
    if standard_basis:
        return out
    n = normal_matrix(m)
    for col, at in enumerate((8, 11, 5)):
        a = v[at:at + 3]
        out[9 + 3 * col: 12 + 3 * col] = (n[0:3] * a[0] + n[3:6] * a[1]) + n[6:9] * a[2]
    return out


def shade_fragments(a, g, tex):
    """the material half of Standard_glTF.shader's fragment stage on interpolated varyings a [18][n]: -> P0, P1, P2 [n, 4], emissive [n, 4] (.w: the occlusion
    texel).  g: the slot as a GLTF record"""
    u, v = a[0], a[1]
    tA = tex.sample(int(g["baseColorSampler"]), u, v)
    tO = tex.sample(int(g["ormSampler"]), u, v)            # one fetch: .z metallic, .y roughness
    tOcc = tex.sample(int(g["occlusionSampler"]), u, v)[..., 0]
    tE = tex.sample(int(g["emissiveSampler"]), u, v)
    tN = tex.sample(int(g["normalSampler"]), u, v)
    base = [(g["baseColorFactor"][c] * tA[..., c]) * a[5 + c] for c in range(4)]      # :389
    metallic, roughness = g["metallicFactor"] * tO[..., 2], g["roughnessFactor"] * tO[..., 1]   # :390-391
    n = ref._normalize(*[f32(2) * tN[..., c] - f32(1) for c in range(3)])
    n = [x * g["normalScale"] for x in n]                                               # :395
    wn = ref._normalize(*[(a[9 + r] * n[0] + a[12 + r] * n[1]) + a[15 + r] * n[2] for r in range(3)])   # :396
    p0 = np.stack([a[2], a[3], a[4], base[3]], -1)
    p1 = np.stack([wn[0], wn[1], wn[2], roughness], -1)
    p2 = np.stack([base[0], base[1], base[2], metallic], -1)
    em = np.stack([g["emissiveFactor"][0] * tE[..., 0], g["emissiveFactor"][1] * tE[..., 1], g["emissiveFactor"][2] * tE[..., 2], tOcc], -1)   # :393, :399
    return p0.astype(f32), p1.astype(f32), p2.astype(f32), em.astype(f32)


def render(scene, prepass=None, rows=None, standard_basis=False):
    """masked_ref.render's result and stats (stats: tested, discarded, nan_alpha, on_cutoff = alphas exactly on their threshold, discarded_at_tie), plus
    gltf bool [n, W] (the pixel's owner is a fragment of a glTF draw), emissive float32 [n, W, 4], ao_out float32 [n, W], ao_in float32 [n, W]"""
    W, H = scene["W"], scene["H"]
    r0, r1 = rows if rows is not None else (0, H)
    V, P = np.asarray(scene["view"], f32).reshape(16), np.asarray(scene["projection"], f32).reshape(16)
    inst, mats = scene["instances"], scene["materials"]
    gmats = mats.view(GLTF)
    tex = MaskedTextures(scene["textures"], scene["srgb"])
    depth = np.zeros((H, W), f32) if prepass is None else np.array(prepass, f32).reshape(H, W).copy()
    ao_in = np.ones((H, W), f32) if scene.get("ao_in") is None else np.asarray(scene["ao_in"], f32).reshape(H, W)
    covered, cutout_owner, gltf_owner = np.zeros((H, W), bool), np.zeros((H, W), bool), np.zeros((H, W), bool)
    order_of = np.zeros((H, W), np.uint64)
    planes = np.empty((3, H, W, 4), f32)
    for k in range(3):
        planes[k] = ref.UNCOVERED[k]
    emissive = np.empty((H, W, 4), f32)
    emissive[:] = NO_EMISSIVE
    ao_out = ao_in.copy()
    stats = dict(cut_one=0, cut_two=0, ties=0, fragments=0, overwritten=0, culled=0, degenerate=0, clipped_away=0, large=0, materials=set(), swapped=0,
                 tested=0, discarded=0, nan_alpha=0, on_cutoff=0, discarded_at_tie=0, gltf_fragments=0)
    prim_base = int(scene.get("prim_base", 0))
    with np.errstate(all="ignore"):
        for draw in scene["draws"]:
            verts, indices = np.asarray(draw["vertices"], f32).reshape(-1, 18), np.asarray(draw["indices"], np.uint32).reshape(-1, 3)
            cutout, gltf = bool(draw.get("alpha_cutout", False)), bool(draw.get("gltf", False))
            nt, ids = len(indices), draw.get("instance_ids")
            first = int(draw.get("first_instance", 0))
            nd = int(draw["num_drawn"]) if draw.get("num_drawn") is not None else (len(ids) if ids is not None else len(inst) - first)
            for d in range(nd):
                i = int(ids[d]) if ids is not None else first + d
                m = np.asarray(inst["model"][i], f32)
                mi = int(inst["materialInstance"][i])
                slot = mi if mi < len(mats) else 0
                material = gmats[slot] if gltf else mats[slot]
                threshold = f32(material["alphaCutoff"]) if gltf else f32(0.5)
                varyings = (lambda q: vertex_varyings(q, m, standard_basis)) if gltf else (lambda q: ref.vertex_varyings(q, m))
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
                        area = ref._to_f32(ref._edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]))
                        l0, l1, l2 = ref._to_f32(e0) / area, ref._to_f32(e1) / area, ref._to_f32(e2) / area
                        z = (Z[0] + (Z[1] - Z[0]) * l1) + (Z[2] - Z[0]) * l2
                        sub = (slice(j0, j1 + 1), slice(i0, i1 + 1))
                        exists = inside & (z > 0) & (z <= 1)
                        passed = exists & (z >= depth[sub])            # GreaterOrEqual, in drawing order
                        if not passed.any():
                            continue
                        av = []
                        for (I, O, tt) in src:
                            aI = varyings(verts[I])
                            av.append(aI if tt is None else aI + (varyings(verts[O]) - aI) * tt)

                        def fragments(mask):
                            q0, q1, q2 = l0[mask] / Wc[0], l1[mask] / Wc[1], l2[mask] / Wc[2]
                            s = (q0 + q1) + q2
                            b0, b1, b2 = q0 / s, q1 / s, q2 / s
                            a = [(av[0][c] * b0 + av[1][c] * b1) + av[2][c] * b2 for c in range(18)]
                            return shade_fragments(a, material, tex) if gltf else ref.shade_fragments(a, material, tex)
                        if cutout:
                            # the discard, before anything of the fragment is written: alpha = P0.w of the very shading that would be written
                            beyond, taps = tex.beyond, dict(tex.taps)
                            alpha = fragments(passed)[0][..., 3]
                            tex.beyond, tex.taps = beyond, taps
                            keep = ~(alpha < threshold)                   # one compare: a NaN on either side survives
                            stats["tested"] += int(alpha.size)
                            stats["discarded"] += int((~keep).sum())
                            stats["nan_alpha"] += int(np.isnan(alpha).sum())
                            stats["on_cutoff"] += int((alpha == threshold).sum())
                            stats["discarded_at_tie"] += int((~keep & (z[passed] == depth[sub][passed])).sum())
                            survivors = np.zeros_like(passed)
                            survivors[passed] = keep
                            passed = survivors
                            if not passed.any():
                                continue
                        stats["fragments"] += int(passed.sum())
                        stats["gltf_fragments"] += int(passed.sum()) if gltf else 0
                        stats["ties"] += int((passed & (z == depth[sub])).sum())
                        stats["overwritten"] += int((passed & covered[sub]).sum())
                        stats["materials"].add(mi)
                        out = fragments(passed)
                        jj, ii = np.nonzero(passed)
                        jj, ii = jj + j0, ii + i0
                        planes[0, jj, ii], planes[1, jj, ii], planes[2, jj, ii] = out[0], out[1], out[2]
                        if gltf:
                            emissive[jj, ii] = out[3]
                            occ, g_ao = out[3][..., 3], ao_in[jj, ii]
                            ao_out[jj, ii] = np.where(occ < g_ao, occ, g_ao)     # GLSL min(x, y) = y < x ? y : x with x = g_AO
                        else:
                            emissive[jj, ii] = NO_EMISSIVE
                            ao_out[jj, ii] = ao_in[jj, ii]
                        depth[jj, ii] = z[passed]
                        covered[jj, ii] = True
                        cutout_owner[jj, ii], gltf_owner[jj, ii] = cutout, gltf
                        order_of[jj, ii] = order + 1
            prim_base += nd * 2 * nt
    stats["beyond_table"], stats["taps"] = tex.beyond, tex.taps
    keys = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order_of
    return dict(planes=planes[:, r0:r1].copy(), depth=depth[r0:r1].copy(), covered=covered[r0:r1].copy(), keys=keys[r0:r1].copy(), stats=stats,
                next_prim_base=prim_base, cutout=cutout_owner[r0:r1].copy(), gltf=gltf_owner[r0:r1].copy(), emissive=emissive[r0:r1].copy(),
                ao_out=ao_out[r0:r1].copy(), ao_in=ao_in[r0:r1].copy())


def composite(radiance, emissive, covered, target):
    """sailor_hip_surface_composite_gltf: covered ? (emissive.rgb + radiance.rgb, radiance.a) : target"""
    out = np.array(target, f32)
    with np.errstate(all="ignore"):
        s = np.concatenate([np.asarray(emissive, f32)[..., :3] + np.asarray(radiance, f32)[..., :3], np.asarray(radiance, f32)[..., 3:]], -1)
    out[covered] = s[covered]
    return out
