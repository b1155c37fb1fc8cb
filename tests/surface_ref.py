"""A float32 NumPy restatement of RenderScene's surface pass (sailor_amd/csrc/surface.hip), written from Content/Shaders/Standard.shader:126-139,
:379-389, :438 and the rules pinned in include/sailor_hip.h.

It is LITERALLY SEQUENTIAL: draw after draw, instance after instance in the order the draw lists them, triangle after triangle, the two parts of a
triangle the near plane cut one after the other, every fragment tested GreaterOrEqual against a depth array and, if it passes, shaded and written at
once.  There are no keys and no maximum in it: the key form of the kernels is checked against the semantics it claims.  (The key it REPORTS per pixel is
put together afterwards from the winner it recorded, so that the kernels' keys can be compared as well.)  Only the pixels of one triangle are worked on at
once, as arrays; every operation is a float32 operation with one rounding, in the order the header states.

A scene is a dict:
  W, H, view (16), projection (16) -- column-major float32
  instances  : sailor_amd.host.INSTANCE_DTYPE records
  materials  : sailor_amd._lib.MATERIAL_DTYPE records
  textures   : list of uint8 [h, w, 4]; srgb: list of bool
  draws      : list of dict(vertices float32 [n, 18] (texcoord 2, position 3, normal 3, tangent 3, bitangent 3, colour 4), indices uint32 [t, 3],
               instance_ids uint32 [m] | None, first_instance, num_drawn, cull_back)
  prim_base  : the first draw's primBase (default 0)
"""
import math

import numpy as np

f32 = np.float32
UNCOVERED = (np.array([0, 0, 0, 0], f32), np.array([0, 0, 1, 1], f32), np.array([0, 0, 0, 0], f32))


def srgb_table():
    """the sRGB transfer function of the 256 byte values in double, rounded once to float32"""
    return np.array([c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4) for c in (i / 255.0 for i in range(256))], np.float64).astype(f32)


def sat_int(x):
    """the device's float -> int conversion: NaN -> 0, saturating at the ends of int32"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0.0, np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def glsl_mul(M, x, y, z, w):
    """mat4 * vec4: ((c0 x + c1 y) + c2 z) + c3 w"""
    return ((M[0:4] * x + M[4:8] * y) + M[8:12] * z) + M[12:16] * w


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def vertex_varyings(v, m):
    """the 18 varyings of Standard.shader:128-138 of one vertex: texcoord, worldPosition, colour, tangentBasis (column by column)"""
    out = np.empty(18, f32)
    out[0:2] = v[0:2]
    wp = glsl_mul(m, v[2], v[3], v[4], f32(1))
    out[2:5] = wp[0:3] / wp[3]
    out[5:9] = v[14:18]
    for col, at in enumerate((8, 11, 5)):   # mat3(inTangent, inBitangent, inNormal)
        a = v[at:at + 3]
        out[9 + 3 * col: 12 + 3 * col] = (m[0:3] * a[0] + m[4:7] * a[1]) + m[8:11] * a[2]
    return out


def _cut(I, dI, O, dO):
    t = dI / (dI - dO)
    return I + (O - I) * t, t


def near_clip(clip, idx):
    """raster_near_clip of the oracle with the vertices' sources: -> list of parts, each (clip [3, 4], sources [(I, O, t | None)] * 3)"""
    d = [clip[k][3] - clip[k][2] for k in range(3)]
    mask = sum(1 << k for k in range(3) if d[k] >= 0)
    plain = lambda k: (idx[k], idx[k], None)
    if mask == 0:
        return []
    if mask == 7:
        return [(np.array(clip), [plain(0), plain(1), plain(2)])]
    one = mask & (mask - 1) == 0
    r = {1: 0, 2: 1, 4: 2}[mask] if one else {6: 1, 5: 2, 3: 0}[mask]
    a, b, c = r, (r + 1) % 3, (r + 2) % 3
    if one:
        AB, tAB = _cut(clip[a], d[a], clip[b], d[b])
        AC, tAC = _cut(clip[a], d[a], clip[c], d[c])
        return [(np.array([clip[a], AB, AC]), [plain(a), (idx[a], idx[b], tAB), (idx[a], idx[c], tAC)])]
    BC, tBC = _cut(clip[b], d[b], clip[c], d[c])
    AC, tAC = _cut(clip[a], d[a], clip[c], d[c])
    return [(np.array([clip[a], clip[b], BC]), [plain(a), plain(b), (idx[b], idx[c], tBC)]),
            (np.array([clip[a], BC, AC]), [plain(a), (idx[b], idx[c], tBC), (idx[a], idx[c], tAC)])]


def setup(clip, src, W, H, cull_back):
    """raster_setup of the oracle: -> (X, Y, Z, w, sources) after the winding swap, or None"""
    X, Y, Z, Wc = [], [], [], []
    for k in range(3):
        c = clip[k]
        if not c[3] > 0:
            return None
        nx, ny, nz = c[0] / c[3], c[1] / c[3], c[2] / c[3]
        xf = (nx + f32(1)) * (f32(W) * f32(0.5))
        yf = (ny + f32(1)) * (f32(H) * f32(-0.5)) + f32(H)
        sx, sy = xf * f32(256), yf * f32(256)
        if not abs(sx) < f32(1.0e9) or not abs(sy) < f32(1.0e9):
            return None
        X.append(int(np.rint(sx))); Y.append(int(np.rint(sy))); Z.append(nz); Wc.append(c[3])
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    if area2 == 0 or (cull_back and area2 > 0):
        return None
    src = list(src)
    if area2 < 0:
        for a in (X, Y, Z, Wc, src):
            a[1], a[2] = a[2], a[1]
    return X, Y, Z, Wc, src


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _top_left(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (dy == 0 and dx > 0) or dy < 0


def _to_f32(e):
    return np.asarray(e, np.int64).astype(f32)   # one rounding, int64 -> float32


class Textures:
    def __init__(self, images, srgb):
        self.images = [np.ascontiguousarray(i, np.uint8) for i in images]
        self.srgb = list(srgb)
        self.table = srgb_table()
        self.beyond = 0   # fetches whose sampler index lay beyond the table
        # what the fetches reached, counted per fragment: uv exactly 0 / 1, below 0 / above 1 / NaN, tap weights of exactly 0 (a texel centre) and 0.5 (a texel
        # edge), the second tap wrapped round to 0, sRGB fetches, fetches through the table's last descriptor
        self.taps = dict(u0=0, u1=0, v0=0, v1=0, below=0, above=0, nan=0, ax0=0, ax_half=0, ay0=0, ay_half=0, wrap_x=0, wrap_y=0, srgb=0, last=0)

    def sample(self, index, u, v):
        """texture(textureSamplers[index], uv): base level, bilinear, Repeat; sRGB decodes r, g, b per tap before the filter -> [n, 4]"""
        if index >= len(self.images):
            self.beyond += 1
            index = 0
        img, srgb = self.images[index], self.srgb[index]
        h, w = img.shape[:2]

        def tap(n, c):
            x = c * f32(n) - f32(0.5)
            fx = np.floor(x)
            i0 = sat_int(fx) % n
            return i0, np.where(i0 + 1 == n, 0, i0 + 1), x - fx
        x0, x1, ax = tap(w, u)
        y0, y1, ay = tap(h, v)
        c = self.taps
        c["u0"] += int((u == 0).sum()); c["u1"] += int((u == 1).sum()); c["v0"] += int((v == 0).sum()); c["v1"] += int((v == 1).sum())
        c["below"] += int(((u < 0) | (v < 0)).sum()); c["above"] += int(((u > 1) | (v > 1)).sum()); c["nan"] += int((np.isnan(u) | np.isnan(v)).sum())
        c["ax0"] += int((ax == 0).sum()); c["ax_half"] += int((ax == f32(0.5)).sum()); c["ay0"] += int((ay == 0).sum()); c["ay_half"] += int((ay == f32(0.5)).sum())
        c["wrap_x"] += int((x1 == 0).sum()); c["wrap_y"] += int((y1 == 0).sum())
        c["srgb"] += int(u.size) if srgb else 0
        c["last"] += int(u.size) if index == len(self.images) - 1 else 0
        out = np.empty(u.shape + (4,), f32)
        for ch in range(4):
            dec = (lambda b: self.table[b]) if (srgb and ch < 3) else (lambda b: b.astype(f32) / f32(255))
            t00, t10, t01, t11 = dec(img[y0, x0, ch]), dec(img[y0, x1, ch]), dec(img[y1, x0, ch]), dec(img[y1, x1, ch])
            top = t00 * (f32(1) - ax) + t10 * ax
            bot = t01 * (f32(1) - ax) + t11 * ax
            out[..., ch] = top * (f32(1) - ay) + bot * ay
        return out


def _normalize(x, y, z):
    l = np.sqrt(dot3(x, y, z, x, y, z))
    return x / l, y / l, z / l


def shade_fragments(a, material, tex):
    """the material half of the fragment stage on interpolated varyings a [18][n] -> P0, P1, P2 [n, 4]"""
    u, v = a[0], a[1]
    tA = tex.sample(int(material["albedoSampler"]), u, v)
    tM = tex.sample(int(material["metalnessSampler"]), u, v)[..., 0]
    tR = tex.sample(int(material["roughnessSampler"]), u, v)[..., 0]
    tN = tex.sample(int(material["normalSampler"]), u, v)
    albedo = [(material["albedo"][c] * tA[..., c]) * a[5 + c] for c in range(4)]   # :383
    metallic, roughness = material["metallic"] * tM, material["roughness"] * tR    # :384-385
    n = _normalize(*[f32(2) * tN[..., c] - f32(1) for c in range(3)])               # :388
    wn = _normalize(*[(a[9 + r] * n[0] + a[12 + r] * n[1]) + a[15 + r] * n[2] for r in range(3)])   # :389
    p0 = np.stack([a[2], a[3], a[4], albedo[3]], -1)
    p1 = np.stack([wn[0], wn[1], wn[2], roughness], -1)
    p2 = np.stack([albedo[0], albedo[1], albedo[2], metallic], -1)
    return p0.astype(f32), p1.astype(f32), p2.astype(f32)


def render(scene, prepass=None, rows=None, perspective=True):
    """-> dict(planes float32 [3, n, W, 4], depth float32 [n, W], covered bool [n, W], keys uint64 [n, W], stats) over the framebuffer rows `rows`
    (default: all).  prepass: the raw depth of the whole frame the pass starts from.  perspective=False is the screen-linear MUTANT (b_k = l_k)."""
    W, H = scene["W"], scene["H"]
    r0, r1 = rows if rows is not None else (0, H)
    V, P = np.asarray(scene["view"], f32).reshape(16), np.asarray(scene["projection"], f32).reshape(16)
    inst, mats = scene["instances"], scene["materials"]
    tex = Textures(scene["textures"], scene["srgb"])
    depth = np.zeros((H, W), f32) if prepass is None else np.array(prepass, f32).reshape(H, W).copy()
    covered = np.zeros((H, W), bool)
    order_of = np.zeros((H, W), np.uint64)
    planes = np.empty((3, H, W, 4), f32)
    for k in range(3):
        planes[k] = UNCOVERED[k]
    stats = dict(cut_one=0, cut_two=0, ties=0, fragments=0, overwritten=0, culled=0, degenerate=0, clipped_away=0, large=0, materials=set(), swapped=0)
    prim_base = int(scene.get("prim_base", 0))
    with np.errstate(all="ignore"):
        for draw in scene["draws"]:
            verts, indices = np.asarray(draw["vertices"], f32).reshape(-1, 18), np.asarray(draw["indices"], np.uint32).reshape(-1, 3)
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
                    clip = [glsl_mul(P, *glsl_mul(V, *glsl_mul(m, verts[q][2], verts[q][3], verts[q][4], f32(1)))) for q in idx]
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
                        # pixel (i, j) has its centre at (256 i + 128, 256 j + 128); // floors
                        i0, i1 = max((min(X) - 128 + 255) // 256, 0), min((max(X) - 128) // 256, W - 1)
                        j0, j1 = max((min(Y) - 128 + 255) // 256, r0), min((max(Y) - 128) // 256, r1 - 1)
                        if i1 < i0 or j1 < j0:
                            continue
                        if (i1 - i0 + 1) * (j1 - j0 + 1) > 64:
                            stats["large"] += 1
                        px, py = np.meshgrid(256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128, 256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)
                        e0, e1, e2 = _edge(X[1], Y[1], X[2], Y[2], px, py), _edge(X[2], Y[2], X[0], Y[0], px, py), _edge(X[0], Y[0], X[1], Y[1], px, py)
                        tl0, tl1, tl2 = _top_left(X[1], Y[1], X[2], Y[2]), _top_left(X[2], Y[2], X[0], Y[0]), _top_left(X[0], Y[0], X[1], Y[1])
                        inside = ~((e0 < 0) | (e1 < 0) | (e2 < 0)) & ~(((e0 == 0) & (not tl0)) | ((e1 == 0) & (not tl1)) | ((e2 == 0) & (not tl2)))
                        area = _to_f32(_edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]))
                        l0, l1, l2 = _to_f32(e0) / area, _to_f32(e1) / area, _to_f32(e2) / area
                        z = (Z[0] + (Z[1] - Z[0]) * l1) + (Z[2] - Z[0]) * l2
                        sub = (slice(j0, j1 + 1), slice(i0, i1 + 1))
                        exists = inside & (z > 0) & (z <= 1)          # a fragment at z == 0 does not exist
                        passed = exists & (z >= depth[sub])            # GreaterOrEqual, in drawing order
                        if not passed.any():
                            continue
                        stats["fragments"] += int(passed.sum())
                        stats["ties"] += int((passed & (z == depth[sub])).sum())
                        stats["overwritten"] += int((passed & covered[sub]).sum())
                        stats["materials"].add(mi)
                        # the varyings of the three vertices (a cut one: aI + (aO - aI) t), then perspective-correct
                        av = []
                        for (I, O, tt) in src:
                            aI = vertex_varyings(verts[I], m)
                            av.append(aI if tt is None else aI + (vertex_varyings(verts[O], m) - aI) * tt)
                        L0, L1, L2 = l0[passed], l1[passed], l2[passed]
                        if perspective:
                            q0, q1, q2 = L0 / Wc[0], L1 / Wc[1], L2 / Wc[2]
                            s = (q0 + q1) + q2
                            b0, b1, b2 = q0 / s, q1 / s, q2 / s
                        else:
                            b0, b1, b2 = L0, L1, L2
                        a = [(av[0][c] * b0 + av[1][c] * b1) + av[2][c] * b2 for c in range(18)]
                        p0, p1, p2 = shade_fragments(a, material, tex)
                        jj, ii = np.nonzero(passed)
                        jj, ii = jj + j0, ii + i0
                        planes[0, jj, ii], planes[1, jj, ii], planes[2, jj, ii] = p0, p1, p2
                        depth[jj, ii] = z[passed]
                        covered[jj, ii] = True
                        order_of[jj, ii] = order + 1
            prim_base += nd * 2 * nt
    stats["beyond_table"], stats["taps"] = tex.beyond, tex.taps
    keys = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | order_of
    return dict(planes=planes[:, r0:r1].copy(), depth=depth[r0:r1].copy(), covered=covered[r0:r1].copy(), keys=keys[r0:r1].copy(), stats=stats,
                next_prim_base=prim_base)


def same_bits_or_class(got, want):
    """per word: equal bits, or both NaN, or both the same infinity"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
