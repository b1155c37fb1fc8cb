"""A float32 NumPy restatement of mip-mapped material textures (sailor_amd/csrc/texture_mips.hip, surface_lod.hip), written from the rules pinned in
include/sailor_hip.h (the mip-mapped section):

  * the chain: level l + 1 from level l -- decode (the sRGB table for r, g, b under the flag, byte / 255 otherwise), sailor_hip_blit_linear's taps, lerp2,
    encode (sRGB: the number of encode-table entries <= x; UNORM: floor(x * 255 + 0.5)) -- next to a float64 twin of every level, which also reports how far
    its value lies from the nearest rounding boundary;
  * the pass: tests/gltf_ref.py's LITERALLY SEQUENTIAL pass (draw after draw, a >= test against a depth array, a discarded fragment dropped before anything of
    it is written) in which every texture() is the trilinear fetch at the implicit level of detail.  The set-up, the clip and the edge functions are
    surface_ref's, the material halves surface_ref.shade_fragments and gltf_ref.shade_fragments, untouched: they call tex.sample(index, u, v), and the sampler
    here holds the fragments' derivatives.  log2 is eye_adaptation_ref.canonical_log2f.  A float64 twin of lambda is reported for the known-answer tests.

A scene is gltf_ref's dict; it may carry `chains` (per texture: the list of its levels, uint8 [h, w, 4]; absent: level 0 alone) and `levels` (per texture: the
descriptor's `levels` field as written, e.g. 0 or 99; absent: the length of the chain)."""
import math

import numpy as np

import gltf_ref
import surface_ref as ref
from eye_adaptation_ref import canonical_log2f
from masked_ref import MaskedTextures
from sailor_amd import _lib
from surface_ref import near_clip, setup

f32, f64 = np.float32, np.float64
GLTF = np.dtype(_lib.GLTF_MATERIAL_DTYPE)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------------
def full_levels(w, h):
    """floor(log2(max(w, h))) + 1 in integers"""
    return int(max(w, h)).bit_length()


def level_count(w, h, levels):
    """n = clamp(levels, 1, full); 0 reads as 1"""
    return 1 if levels < 1 else min(int(levels), full_levels(w, h))


def level_extent(e, l):
    return max(e >> l, 1)


def chain_offset(w, h, l):
    """sailor_hip_mip_chain_texels(w, h, l)"""
    return sum(level_extent(w, k) * level_extent(h, k) for k in range(l))


def srgb_decode64(c):
    return c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4)


def encode_table64():
    """the 255 rounding boundaries of the sRGB encode in double: the decode of (k - 0.5) / 255"""
    return np.array([srgb_decode64((k - 0.5) / 255.0) for k in range(1, 256)], f64)


def encode_table():
    return encode_table64().astype(f32)


def _axis_taps(ns, nd, f):
    """bilinear_taps along one axis for the nd destination texels over ns source texels, in the float type f -> (i0, i1, weight)"""
    u = (np.arange(nd).astype(f) + f(0.5)) / f(nd)
    x = u * f(ns) - f(0.5)
    fx = np.floor(x)
    x0 = fx.astype(np.int64)
    return np.clip(x0, 0, ns - 1), np.clip(x0, -1, ns - 2) + 1, (x - fx).astype(f)


def _filtered(img, f, decode):
    """the four taps of every texel of the next level, decoded per channel by decode(bytes, ch), under lerp2 in the float type f -> [hd, wd, 4]"""
    hs, ws = img.shape[:2]
    wd, hd = level_extent(ws, 1), level_extent(hs, 1)
    x0, x1, ax = _axis_taps(ws, wd, f)
    y0, y1, ay = _axis_taps(hs, hd, f)
    ax, ay = ax[None, :], ay[:, None]
    out = np.empty((hd, wd, 4), f)
    for ch in range(4):
        t00, t10 = decode(img[np.ix_(y0, x0)][..., ch], ch), decode(img[np.ix_(y0, x1)][..., ch], ch)
        t01, t11 = decode(img[np.ix_(y1, x0)][..., ch], ch), decode(img[np.ix_(y1, x1)][..., ch], ch)
        top = t00 * (f(1) - ax) + t10 * ax
        bot = t01 * (f(1) - ax) + t11 * ax
        out[..., ch] = top * (f(1) - ay) + bot * ay
    return out


def next_level(img, srgb):
    """level l + 1 of level l (uint8 [h, w, 4]), every operation one float32 rounding"""
    img = np.ascontiguousarray(img, np.uint8)
    table, enc = ref.srgb_table(), encode_table()
    x = _filtered(img, f32, lambda b, ch: table[b] if (srgb and ch < 3) else b.astype(f32) / f32(255))
    out = np.empty(x.shape, np.uint8)
    for ch in range(4):
        if srgb and ch < 3:
            out[..., ch] = np.searchsorted(enc, x[..., ch], side="right")          # the number of entries <= x
        else:
            out[..., ch] = np.floor(x[..., ch] * f32(255) + f32(0.5))
    return out


def next_level64(img, srgb):
    """the float64 twin of next_level -> (bytes uint8 [h, w, 4], margin float64 [h, w, 4]): the distance of the double value from the nearest rounding
    boundary, as a fraction of the spacing of the boundaries there"""
    img = np.ascontiguousarray(img, np.uint8)
    table64 = np.array([srgb_decode64(i / 255.0) for i in range(256)], f64)
    enc = encode_table64()
    x = _filtered(img, f64, lambda b, ch: table64[b] if (srgb and ch < 3) else b.astype(f64) / 255.0)
    out, margin = np.empty(x.shape, np.uint8), np.empty(x.shape, f64)
    for ch in range(4):
        v = x[..., ch]
        if srgb and ch < 3:
            k = np.searchsorted(enc, v, side="right")
            out[..., ch] = k
            below, above = enc[np.clip(k - 1, 0, 254)], enc[np.clip(k, 0, 254)]
            spacing = np.where((k > 0) & (k < 255), above - below, np.where(k == 0, enc[1] - enc[0], enc[254] - enc[253]))
            margin[..., ch] = np.minimum(np.where(k > 0, np.abs(v - below), np.inf), np.where(k < 255, np.abs(above - v), np.inf)) / spacing
        else:
            s = v * 255.0 + 0.5
            out[..., ch] = np.floor(s)
            margin[..., ch] = np.abs(s - np.rint(s))            # the boundaries are 1 / 255 apart: in units of that spacing
    return out, margin


def build_chain(img, srgb, levels=None):
    """the levels of a texture, level 0 = img: what sailor_hip_texture_generate_mips leaves behind `texels`"""
    img = np.ascontiguousarray(img, np.uint8)
    n = full_levels(img.shape[1], img.shape[0]) if levels is None else levels
    chain = [img]
    for _ in range(n - 1):
        chain.append(next_level(chain[-1], srgb))
    return chain


def flat_chain(chain):
    """the chain as the uint32 texels behind a descriptor"""
    return np.concatenate([np.ascontiguousarray(l, np.uint8).view(np.uint32).reshape(-1) for l in chain])


# ---- the level of detail --------------------------------------------------------------------------------------------------------------------------------
def scale_factor(w, h, d):
    """rule 4: r2 of a w x h descriptor from the derivatives d = (dudx, dvdx, dudy, dvdy), float32 arrays"""
    fw, fh = f32(w), f32(h)
    ax, bx, ay, by = d[0] * fw, d[1] * fh, d[2] * fw, d[3] * fh
    rx, ry = ax * ax + bx * bx, ay * ay + by * by
    return np.where(ry > rx, ry, rx).astype(f32)


def select_levels(w, h, n, d):
    """rule 5 -> (hi int [m], delta float32 [m], blend bool [m]); blend False: level hi alone"""
    m = np.shape(d[0])
    hi, delta, blend = np.zeros(m, np.int64), np.zeros(m, f32), np.zeros(m, bool)
    if n <= 1:
        return hi, delta, blend
    with np.errstate(all="ignore"):
        r2 = scale_factor(w, h, d)
        minified = r2 > f32(1.0)
        last = minified & (r2 >= f32(4.0 ** (n - 1)))
        mid = minified & ~last
        lam = f32(0.5) * canonical_log2f(np.where(mid, r2, f32(2.0)))
        k = lam.astype(np.int64)                                   # (int)lambda
        beyond = mid & (k >= n - 1)
        blend = mid & ~beyond
        hi = np.where(last | beyond, n - 1, np.where(blend, k, 0))
        delta = np.where(blend, lam - k.astype(f32), f32(0)).astype(f32)
    return hi, delta, blend


def lambda64(w, h, d):
    """the float64 twin of lambda over the same float32 derivatives: 0.5 log2(max(rx, ry))"""
    d = [np.asarray(q, f32).astype(f64) for q in d]
    rx, ry = (d[0] * w) ** 2 + (d[1] * h) ** 2, (d[2] * w) ** 2 + (d[3] * h) ** 2
    with np.errstate(all="ignore"):
        return 0.5 * np.log2(np.maximum(rx, ry))


class LodTextures:
    """the table of mip-mapped descriptors.  sample(index, u, v) is texture() at the implicit level of detail of the fragments whose derivatives `derivs`
    holds; each level is fetched by surface_ref.Textures.sample (masked_ref's: a descriptor without texels samples 0) over that level's extents."""

    def __init__(self, images, srgb, chains=None, levels=None):
        self.count = len(images)
        self.chains = [[np.ascontiguousarray(i, np.uint8)] if chains is None or chains[k] is None else [np.ascontiguousarray(l, np.uint8) for l in chains[k]]
                       for k, i in enumerate(images)]
        self.fields = [len(c) for c in self.chains] if levels is None else [int(x) for x in levels]
        self.level = [[MaskedTextures([l], [s]) for l in c] for c, s in zip(self.chains, srgb)]
        self.derivs, self.pixels = None, None     # of the fragments being shaded: (dudx, dvdx, dudy, dvdy) and (columns, framebuffer rows)
        self.beyond, self.taps = 0, {}
        self.fetched = {}     # (descriptor, level) -> fragments that fetched it
        self.lambdas = []     # (descriptor, columns, rows, lambda32, lambda64) of the fragments that blended two levels

    def sample(self, index, u, v):
        at = index if index < self.count else 0
        self.beyond += int(index >= self.count)
        base = self.chains[at][0]
        h, w = base.shape[:2]
        if h == 0 or w == 0:
            return np.zeros(np.shape(u) + (4,), f32)
        n = level_count(w, h, self.fields[at])
        assert n <= len(self.chains[at]), f"descriptor {at} announces {n} levels and holds {len(self.chains[at])}"
        fetch = lambda l, sel: self.level[at][l].sample(0, u[sel], v[sel])
        if n == 1:
            self.fetched[(at, 0)] = self.fetched.get((at, 0), 0) + int(np.size(u))
            return fetch(0, Ellipsis)
        hi, delta, blend = select_levels(w, h, n, self.derivs)
        if blend.any():
            lam32 = f32(0.5) * canonical_log2f(scale_factor(w, h, [q[blend] for q in self.derivs]))
            self.lambdas.append((at, self.pixels[0][blend], self.pixels[1][blend], lam32, lambda64(w, h, [q[blend] for q in self.derivs])))
        out = np.empty(np.shape(u) + (4,), f32)
        for l in np.unique(hi):
            sel = hi == l
            t = fetch(int(l), sel)
            self.fetched[(at, int(l))] = self.fetched.get((at, int(l)), 0) + int(sel.sum())
            b = sel & blend
            if b.any():
                two = blend[sel]
                dl = delta[b][:, None]
                t[two] = t[two] * (f32(1) - dl) + fetch(int(l) + 1, b) * dl
                self.fetched[(at, int(l) + 1)] = self.fetched.get((at, int(l) + 1), 0) + int(b.sum())
            out[sel] = t
        return out


def _uv_at(av, X, Y, Wc, area, px, py):
    """(a[0], a[1]) of the varying formula at the centres (px, py), inside the triangle or not"""
    e0, e1, e2 = ref._edge(X[1], Y[1], X[2], Y[2], px, py), ref._edge(X[2], Y[2], X[0], Y[0], px, py), ref._edge(X[0], Y[0], X[1], Y[1], px, py)
    l0, l1, l2 = ref._to_f32(e0) / area, ref._to_f32(e1) / area, ref._to_f32(e2) / area
    q0, q1, q2 = l0 / Wc[0], l1 / Wc[1], l2 / Wc[2]
    s = (q0 + q1) + q2
    b0, b1, b2 = q0 / s, q1 / s, q2 / s
    return [(av[0][c] * b0 + av[1][c] * b1) + av[2][c] * b2 for c in range(2)]


def derivatives(av, X, Y, Wc, area, ii, jj):
    """rule 3 at the pixels (ii, jj) (jj = framebuffer rows): d/dx = uv(i | 1, j) - uv(i & ~1, j), d/dy = uv(i, j | 1) - uv(i, j & ~1)"""
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    c = lambda q: 256 * q + 128
    right, left = _uv_at(av, X, Y, Wc, area, c(ii | 1), c(jj)), _uv_at(av, X, Y, Wc, area, c(ii & ~1), c(jj))
    down, up = _uv_at(av, X, Y, Wc, area, c(ii), c(jj | 1)), _uv_at(av, X, Y, Wc, area, c(ii), c(jj & ~1))
    return (right[0] - left[0]).astype(f32), (right[1] - left[1]).astype(f32), (down[0] - up[0]).astype(f32), (down[1] - up[1]).astype(f32)


# ---- the pass -------------------------------------------------------------------------------------------------------------------------------------------
def render(scene, prepass=None, rows=None):
    """gltf_ref.render's result (planes, depth, covered, keys, cutout, gltf, emissive, ao_out, ao_in, next_prim_base) with every fetch at its implicit level
    of detail; stats: tested, discarded, fragments, fetched {(descriptor, level): fragments}, lambdas, alpha float32 [n, W] (the alpha a cutout owner was tested
    with), threshold float32 [n, W]"""
    W, H = scene["W"], scene["H"]
    r0, r1 = rows if rows is not None else (0, H)
    V, P = np.asarray(scene["view"], f32).reshape(16), np.asarray(scene["projection"], f32).reshape(16)
    inst, mats = scene["instances"], scene["materials"]
    gmats = mats.view(GLTF)
    tex = LodTextures(scene["textures"], scene["srgb"], scene.get("chains"), scene.get("levels"))
    depth = np.zeros((H, W), f32) if prepass is None else np.array(prepass, f32).reshape(H, W).copy()
    ao_in = np.ones((H, W), f32) if scene.get("ao_in") is None else np.asarray(scene["ao_in"], f32).reshape(H, W)
    covered, cutout_owner, gltf_owner = np.zeros((H, W), bool), np.zeros((H, W), bool), np.zeros((H, W), bool)
    order_of = np.zeros((H, W), np.uint64)
    planes = np.empty((3, H, W, 4), f32)
    for k in range(3):
        planes[k] = ref.UNCOVERED[k]
    emissive = np.empty((H, W, 4), f32)
    emissive[:] = gltf_ref.NO_EMISSIVE
    ao_out = ao_in.copy()
    tested_alpha, tested_threshold = np.full((H, W), np.nan, f32), np.full((H, W), np.nan, f32)
    stats = dict(tested=0, discarded=0, fragments=0, cut_two=0, cut_one=0, helpers_outside=0, helpers_off_frame=0, nonfinite_derivs=0)
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
                varyings = (lambda q: gltf_ref.vertex_varyings(q, m)) if gltf else (lambda q: ref.vertex_varyings(q, m))
                for t in range(nt):
                    idx = [int(q) for q in indices[t]]
                    clip = [ref.glsl_mul(P, *ref.glsl_mul(V, *ref.glsl_mul(m, verts[q][2], verts[q][3], verts[q][4], f32(1)))) for q in idx]
                    parts = near_clip(clip, idx)
                    stats["cut_two"] += int(len(parts) == 2)
                    stats["cut_one"] += int(len(parts) == 1 and any(s[2] is not None for s in parts[0][1]))
                    for part, (pc, src) in enumerate(parts):
                        order = prim_base + d * 2 * nt + 2 * t + part
                        su = setup(pc, src, W, H, draw.get("cull_back", False))
                        if su is None:
                            continue
                        X, Y, Z, Wc, src = su
                        i0, i1 = max((min(X) - 128 + 255) // 256, 0), min((max(X) - 128) // 256, W - 1)
                        j0, j1 = max((min(Y) - 128 + 255) // 256, r0), min((max(Y) - 128) // 256, r1 - 1)
                        if i1 < i0 or j1 < j0:
                            continue
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

                        def fragments(mask, count=False):
                            q0, q1, q2 = l0[mask] / Wc[0], l1[mask] / Wc[1], l2[mask] / Wc[2]
                            s = (q0 + q1) + q2
                            b0, b1, b2 = q0 / s, q1 / s, q2 / s
                            a = [(av[0][c] * b0 + av[1][c] * b1) + av[2][c] * b2 for c in range(18)]
                            jj, ii = np.nonzero(mask)
                            jj, ii = jj + j0, ii + i0
                            tex.derivs, tex.pixels = derivatives(av, X, Y, Wc, area, ii, jj), (ii, jj)
                            if count:
                                stats["nonfinite_derivs"] += int((~np.isfinite(np.stack(tex.derivs))).any(0).sum())
                                for mi_, mj_ in ((ii ^ 1, jj), (ii, jj ^ 1)):
                                    stats["helpers_off_frame"] += int(((mi_ >= W) | (mj_ >= H)).sum())
                                    h0, h1, h2 = (ref._edge(X[a_], Y[a_], X[b_], Y[b_], 256 * mi_ + 128, 256 * mj_ + 128) for a_, b_ in ((1, 2), (2, 0), (0, 1)))
                                    stats["helpers_outside"] += int(((h0 < 0) | (h1 < 0) | (h2 < 0)).sum())
                            return gltf_ref.shade_fragments(a, material, tex) if gltf else ref.shade_fragments(a, material, tex)
                        if cutout:
                            fetched, lambdas = dict(tex.fetched), list(tex.lambdas)
                            alpha = fragments(passed)[0][..., 3]          # P0.w of the very shading that would be written
                            tex.fetched, tex.lambdas = fetched, lambdas
                            keep = ~(alpha < threshold)                   # one compare: a NaN on either side survives
                            stats["tested"] += int(alpha.size)
                            stats["discarded"] += int((~keep).sum())
                            survivors = np.zeros_like(passed)
                            survivors[passed] = keep
                            passed = survivors
                            if not passed.any():
                                continue
                        stats["fragments"] += int(passed.sum())
                        out = fragments(passed, count=True)
                        jj, ii = np.nonzero(passed)
                        jj, ii = jj + j0, ii + i0
                        planes[0, jj, ii], planes[1, jj, ii], planes[2, jj, ii] = out[0], out[1], out[2]
                        if gltf:
                            emissive[jj, ii] = out[3]
                            occ, g_ao = out[3][..., 3], ao_in[jj, ii]
                            ao_out[jj, ii] = np.where(occ < g_ao, occ, g_ao)
                        else:
                            emissive[jj, ii] = gltf_ref.NO_EMISSIVE
                            ao_out[jj, ii] = ao_in[jj, ii]
                        depth[jj, ii] = z[passed]
                        covered[jj, ii] = True
                        cutout_owner[jj, ii], gltf_owner[jj, ii] = cutout, gltf
                        tested_alpha[jj, ii], tested_threshold[jj, ii] = (out[0][..., 3], threshold) if cutout else (np.nan, np.nan)
                        order_of[jj, ii] = order + 1
            prim_base += nd * 2 * nt
    stats.update(fetched=tex.fetched, lambdas=tex.lambdas, beyond_table=tex.beyond, alpha=tested_alpha[r0:r1].copy(), threshold=tested_threshold[r0:r1].copy())
    keys = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order_of
    return dict(planes=planes[:, r0:r1].copy(), depth=depth[r0:r1].copy(), covered=covered[r0:r1].copy(), keys=keys[r0:r1].copy(), stats=stats,
                next_prim_base=prim_base, cutout=cutout_owner[r0:r1].copy(), gltf=gltf_owner[r0:r1].copy(), emissive=emissive[r0:r1].copy(),
                ao_out=ao_out[r0:r1].copy(), ao_in=ao_in[r0:r1].copy())
