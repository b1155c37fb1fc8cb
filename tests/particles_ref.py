"""ExperimentalParticles restated in NumPy (sailor_amd/csrc/particles.hip), from ComputeParticles.shader:85-137, Particle.shader:117-136 and :241-253,
Lighting.glsl:168-196 and :242-261 and the rules pinned in include/sailor_hip.h.

Every stage is written ONCE over a number type T: with T = float32 it is the shader's operation order with one rounding per operation (what the kernels
are held to bit for bit wherever no library function enters); with T = float64 it is the reference the kernels' values are bounded against, computed from
the same fp32 inputs.  What is discrete is pinned and taken over by the float64 form unchanged: the frame and record indices (32-bit unsigned, wrapping),
the snapped vertices, coverage and the owning primitive of a pixel.  Every other discrete decision carries its conditioning -- the distance of the deciding
quantity from its threshold -- so that a test knows where float64 decides the outcome and where fp32 may legitimately land on the other side:
  update : `gate` length(axis) > 0 with `alen`, `enabled` > 0.5 with its margin, `from_up` the angle between the direction and +-up
  shade  : `early` the PCF early-outs with `early_margin`, `tap_margin` the smallest |currentDepth + bias - pcfDepth| of the sixteen taps, and the
           selections max(0, dot), min(lighting, shadow), max(0.05, .) with `sel_margin`
The rasteriser is tests/surface_ref.py's (near_clip, setup, the edge functions): sequential, primitive after primitive.
"""
import numpy as np

import surface_ref as sr
from oracle.oracle_f64 import POISSON as _POISSON
from sailor_amd import _lib

f32, f64 = np.float32, np.float64
POISSON = np.asarray(_POISSON, f32)            # Lighting.glsl:176-185, fp32 literals
BIAS = f32(0.00001)                            # Particle.shader:251
M32 = np.uint64(0xFFFFFFFF)
INSTANCE_DTYPE = np.dtype(_lib.PARTICLE_INSTANCE_DTYPE)
RECORD_DTYPE = np.dtype(_lib.PARTICLE_DATA_DTYPE)

# ---- the bounds of tests/test_particles_gpu.py ------------------------------------------------------------------------------------------------------
# E_REF_*: the worst deviation of the fp32 restatement from float64 over the generic update cases (directions at least 1e-2 rad from +-up, p1 != p2), per
# matrix in units of 2^-23 x that matrix's largest magnitude, per colour in units of 2^-23 x that colour's largest magnitude; measured by
# tests/test_particles_cpu.py::test_fp32_update_against_float64, which asserts the measurement itself (E_MEASURED within the allowance, both ways).  The GPU is
# held to 4 x E_REF: the device library's
# sinf / cosf / acosf / powf and the host's differ by a few ulp per call, and the error passes through two 4 x 4 products.
E_MEASURED_MATRIX = 3.263   # U6: the trail's decay through both products
E_MEASURED_COLOUR = 0.222   # U1 at frame 3: alpha * decay, one product and powf
LIBM_ALLOWANCE = 1.03       # another host's pow / sin / cos / acos may round a last bit the other way: 3 %, and the CPU test holds the measurement to it both ways
E_REF_MATRIX = E_MEASURED_MATRIX * LIBM_ALLOWANCE
E_REF_COLOUR = E_MEASURED_COLOUR * LIBM_ALLOWANCE
GPU_BOUND_FACTOR = 4.0      # the GPU bounds: 13.44 (matrix), 0.915 (colour)
# what the GPU showed (tests/test_particles_gpu.py prints it): see DESIGN.md section 4, ExperimentalParticles
GPU_OBSERVED_MATRIX = 3.263   # U6, the same instance as on the host
GPU_OBSERVED_COLOUR = 0.222   # U1 at frame 3
GENERIC_MIN_ANGLE = 1e-2
# a discontinuous decision of the fragment stage counts as decided by float64 where its margin exceeds these (fp32 spacing on [0.5, 1] is 6e-8; the
# receivers of tests/particles_cases.py sit 1e-3 behind their occluders against a bias of 1e-5)
TAP_DECIDED = 1e-6
EARLY_DECIDED = 1e-5
MAIN_RELATIVE = 1e-4
MAX_UNDECIDED_FRACTION = 0.02


def cvt_u32(x):
    """uint(f) as the device converts: NaN and negatives -> 0, saturating at 2^32 - 1"""
    x = np.asarray(x, f64)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.minimum(np.floor(x), 4294967295.0), 0.0).astype(np.uint64)


def glsl_mod(x, y):
    return x - y * np.floor(x / y)


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def mat_mul(A, B):
    """[n, 16] x [n, 16], column-major, GLSL: column j = ((a0 b0j + a1 b1j) + a2 b2j) + a3 b3j"""
    out = np.empty_like(A)
    for j in range(4):
        b = [B[:, 4 * j + k, None] for k in range(4)]
        out[:, 4 * j: 4 * j + 4] = ((A[:, 0:4] * b[0] + A[:, 4:8] * b[1]) + A[:, 8:12] * b[2]) + A[:, 12:16] * b[3]
    return out


def identity(n, T):
    m = np.zeros((n, 16), T)
    m[:, [0, 5, 10, 15]] = 1
    return m


def record_indices(pc, current_time):
    """-> frame, current [n], iNew [n], iOld [n]: ComputeParticles.shader:100-107; the float steps are fp32 whatever T is (they are index arithmetic)"""
    n, nf, fps, tf = int(pc.numInstances), int(pc.numFrames), int(pc.fps), int(pc.traceFrames)
    with np.errstate(all="ignore"):
        frame = cvt_u32(glsl_mod(f32(current_time) * f32(fps), f32(nf)))
        ids = np.arange(n, dtype=np.uint64)
        current = cvt_u32(glsl_mod(ids.astype(f32), f32(tf)))
        tail = ids // np.uint64(tf)
        i_new = (((((frame - current) & M32) * np.uint64(n)) & M32) // np.uint64(tf) + tail) & M32
        i_old = (((((frame - current - np.uint64(1)) & M32) * np.uint64(n)) & M32) // np.uint64(tf) + tail) & M32
    return int(frame), current, i_new, i_old


def fetch(records, index):
    """records[index] as [n, 20] float32; an index at or past the end reads the all-zero record"""
    flat = np.ascontiguousarray(records).view(f32).reshape(-1, 20)
    out = np.zeros((len(index), 20), f32)
    ok = index < np.uint64(len(flat))
    out[ok] = flat[index[ok].astype(np.int64)]
    return out, ~ok


def update(records, pc, current_time, T=f32):
    """-> dict(model [n, 16], color [n, 4], colorOld [n, 4] in T; isCulled; the conditioning; the indices)"""
    frame, current, i_new, i_old = record_indices(pc, current_time)
    new32, zero_new = fetch(records, i_new)
    old32, zero_old = fetch(records, i_old)
    new, old = new32.astype(T), old32.astype(T)
    n = len(current)
    zero, one = T(0), T(1)
    with np.errstate(all="ignore"):
        decay = np.power(T(f32(pc.traceDecay)), current.astype(T)).astype(T)
        x1, y1, z1, x2, y2, z2 = new[:, 4], new[:, 5], new[:, 6], new[:, 12], new[:, 13], new[:, 14]
        ex, ey, ez = x2 - x1, y2 - y1, z2 - z1
        dist = np.sqrt(dot3(ex, ey, ez, ex, ey, ez))
        dx, dy, dz = ex / dist, ey / dist, ez / dist
        ax, ay, az = zero * dz - dy * one, one * dx - dz * zero, zero * dy - dx * zero
        cosine = (zero * dx + zero * dy) + one * dz
        angle = np.arccos(cosine).astype(T)
        alen = np.sqrt(dot3(ax, ay, az, ax, ay, az))
        gate = alen > 0
        c, s = np.cos(angle).astype(T), np.sin(angle).astype(T)
        omc = one - c
        ux, uy, uz = ax / alen, ay / alen, az / alen
        rot = {0: c + ux * ux * omc, 1: ux * uy * omc - uz * s, 2: ux * uz * omc + uy * s,
               4: uy * ux * omc + uz * s, 5: c + uy * uy * omc, 6: uy * uz * omc - ux * s,
               8: uz * ux * omc - uy * s, 9: uz * uy * omc + ux * s, 10: c + uz * uz * omc}
        R = identity(n, T)
        for k, v in rot.items():
            R[:, k] = np.where(gate, v, R[:, k])
        S = identity(n, T)
        S[:, 10] = dist
        S[:, 0] = S[:, 5] = new[:, 2] * decay * T(1.5)
        Tm = identity(n, T)
        Tm[:, 12], Tm[:, 13], Tm[:, 14] = (x1 + x2) * T(0.5), (y1 + y2) * T(0.5), (z1 + z2) * T(0.5)
        model = mat_mul(mat_mul(Tm, R), S)
        color = np.stack([new[:, 16], new[:, 17], new[:, 18], new[:, 19] * decay], 1)
        color_old = np.stack([old[:, 16], old[:, 17], old[:, 18], old[:, 19] * decay], 1)
        from_up = np.minimum(np.arccos(np.clip(dz.astype(f64), -1, 1)), np.pi - np.arccos(np.clip(dz.astype(f64), -1, 1)))
    return dict(model=model, color=color, colorOld=color_old, isCulled=(new32[:, 0] > f32(0.5)).astype(np.uint32), gate=gate, alen=alen, angle=angle,
                from_up=from_up, degenerate=~(dist > 0), enabled_margin=np.abs(new32[:, 0].astype(f64) - 0.5), decay=decay, frame=frame, current=current,
                i_new=i_new, i_old=i_old, zero_new=zero_new, zero_old=zero_old, dist=dist)


def apply_update(before, out):
    """the instance buffer after the update: the first 96 bytes and isCulled written, materialInstance and the padding as they were"""
    after = np.array(before, dtype=INSTANCE_DTYPE, copy=True)
    after["model"], after["color"], after["colorOld"], after["isCulled"] = out["model"].astype(f32), out["color"].astype(f32), out["colorOld"].astype(f32), out["isCulled"]
    return after


def generic(out):
    """the instances whose matrix and colours are compared to float64: a direction at least GENERIC_MIN_ANGLE from +-up, p1 != p2 (out: the float64 form)"""
    return ~out["degenerate"] & (out["from_up"] >= GENERIC_MIN_ANGLE)


def deviation(got, want):
    """per instance: max |got - want| over the entries, in units of 2^-23 x the largest magnitude of the float64 entries"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    scale = np.abs(want).max(axis=1)
    with np.errstate(all="ignore"):
        return np.where(scale > 0, np.abs(got - want).max(axis=1) / (2.0 ** -23 * scale), np.where(np.abs(got - want).max(axis=1) == 0, 0.0, np.inf))


# ---- the two passes -----------------------------------------------------------------------------------------------------------------------------------
def _mul1(A, B):
    return mat_mul(np.asarray(A).reshape(1, 16), np.asarray(B).reshape(1, 16))[0]


def raster(models, verts, indices, W, H, light_matrix=None, projection=None, view=None, depth0=None):
    """every instance, triangle and part in primitive order, fp32.  light_matrix: the shadow pass -- clip = (L * model) * p, no depth test, the LAST
    primitive owns a texel (-> `map`, untouched texels 0).  projection / view: the colour pass -- GreaterOrEqual against depth0 (-> `depth`).
    -> dict(map | depth, owner uint32 [H, W] = order + 1 or 0, prims {order: set-up}, stats)"""
    shadow = light_matrix is not None
    out = np.zeros((H, W), f32) if shadow else np.array(depth0, f32).reshape(H, W).copy()
    owner = np.zeros((H, W), np.uint32)
    prims = {}
    stats = dict(cut_one=0, cut_two=0, clipped_away=0, degenerate=0, culled=0, fragments=0, later_farther=0, z_outside=0, ties=0, depth_failed=0, large=0)
    nt = len(indices)
    with np.errstate(all="ignore"):
        for i, m in enumerate(np.asarray(models, f32).reshape(-1, 16)):
            LM = _mul1(np.asarray(light_matrix, f32), m) if shadow else None
            for t in range(nt):
                idx = [int(q) for q in indices[t]]
                if shadow:
                    clip = [sr.glsl_mul(LM, verts[q][2], verts[q][3], verts[q][4], f32(1)) for q in idx]
                else:
                    clip = [sr.glsl_mul(projection, *sr.glsl_mul(view, *sr.glsl_mul(m, verts[q][2], verts[q][3], verts[q][4], f32(1)))) for q in idx]
                parts = sr.near_clip(clip, idx)
                stats["clipped_away"] += not parts
                stats["cut_two"] += len(parts) == 2
                stats["cut_one"] += len(parts) == 1 and any(s[2] is not None for s in parts[0][1])
                for part, (pc, src) in enumerate(parts):
                    order = (i * nt + t) * 2 + part
                    su = sr.setup(pc, src, W, H, True)
                    if su is None:
                        stats["culled" if sr.setup(pc, src, W, H, False) is not None else "degenerate"] += 1
                        continue
                    X, Y, Z, Wc, src = su
                    i0, i1 = max((min(X) - 128 + 255) // 256, 0), min((max(X) - 128) // 256, W - 1)
                    j0, j1 = max((min(Y) - 128 + 255) // 256, 0), min((max(Y) - 128) // 256, H - 1)
                    if i1 < i0 or j1 < j0:
                        continue
                    stats["large"] += (i1 - i0 + 1) * (j1 - j0 + 1) > 64
                    px, py = np.meshgrid(256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128, 256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)
                    e0, e1, e2 = sr._edge(X[1], Y[1], X[2], Y[2], px, py), sr._edge(X[2], Y[2], X[0], Y[0], px, py), sr._edge(X[0], Y[0], X[1], Y[1], px, py)
                    tl0, tl1, tl2 = sr._top_left(X[1], Y[1], X[2], Y[2]), sr._top_left(X[2], Y[2], X[0], Y[0]), sr._top_left(X[0], Y[0], X[1], Y[1])
                    inside = ~((e0 < 0) | (e1 < 0) | (e2 < 0)) & ~(((e0 == 0) & (not tl0)) | ((e1 == 0) & (not tl1)) | ((e2 == 0) & (not tl2)))
                    area = sr._to_f32(sr._edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]))
                    l1, l2 = sr._to_f32(e1) / area, sr._to_f32(e2) / area
                    z = (Z[0] + (Z[1] - Z[0]) * l1) + (Z[2] - Z[0]) * l2
                    sub = (slice(j0, j1 + 1), slice(i0, i1 + 1))
                    exists = inside & (z > 0) & (z <= 1)
                    stats["z_outside"] += int((inside & ~exists).sum())
                    if shadow:
                        passed = exists
                        stats["later_farther"] += int((passed & (owner[sub] != 0) & (z < out[sub])).sum())
                    else:
                        passed = exists & (z >= out[sub])
                        stats["ties"] += int((passed & (z == out[sub])).sum())
                        stats["depth_failed"] += int((exists & ~passed).sum())
                    if not passed.any():
                        continue
                    stats["fragments"] += int(passed.sum())
                    jj, ii = np.nonzero(passed)
                    out[jj + j0, ii + i0] = z[passed]
                    owner[jj + j0, ii + i0] = order + 1
                    prims[order] = dict(X=X, Y=Y, Z=Z, w=Wc, src=src, inst=i, tri=t, part=part)
    return {"map" if shadow else "depth": out, "owner": owner, "prims": prims, "stats": stats}


def _vec(M, x, y, z, w):
    """mat4 * vec4 over arrays: four arrays"""
    return [((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w for r in range(4)]


def vertex_varyings(v, inst, T):
    """the ten varyings of one vertex (Particle.shader:119-135): worldPosition, color = mix(color, colorOld, (p.z + 1) / 2), mat3(model) * inNormal"""
    v = np.asarray(v, f32).astype(T)
    m, color, old = np.asarray(inst["model"], f32).astype(T), np.asarray(inst["color"], f32).astype(T), np.asarray(inst["colorOld"], f32).astype(T)
    out = np.empty(10, T)
    wp = _vec(m, v[2], v[3], v[4], T(1))
    out[0:3] = [wp[0] / wp[3], wp[1] / wp[3], wp[2] / wp[3]]
    a = (v[4] + T(1)) / T(2)
    out[3:7] = color * (T(1) - a) + old * a
    out[7:10] = (m[0:3] * v[5] + m[4:7] * v[6]) + m[8:11] * v[7]
    return out


def sample_map(smap, u, v, T):
    """texture(shadowMapSampler, uv).r: bilinear, Clamp (sampling.h bilinear_taps + lerp2) -> the sample, and whether a tap index was clamped"""
    H, W = smap.shape
    x, y = u * T(W) - T(0.5), v * T(H) - T(0.5)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    x0, y0 = sr.sat_int(fx), sr.sat_int(fy)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0, -1, W - 2) + 1
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0, -1, H - 2) + 1
    m = smap.astype(T)
    top = m[ya, xa] * (T(1) - ax) + m[ya, xb] * ax
    bot = m[yb, xa] * (T(1) - ax) + m[yb, xb] * ax
    return top * (T(1) - ay) + bot * ay, (x0 < 0) | (x0 > W - 2) | (y0 < 0) | (y0 > H - 2)


def shadow_pcf(smap, lp, T):
    """ShadowCalculation_Pcf + ManualPCF (Lighting.glsl:242-261, :168-196) -> shadow, dict(early, early_x, early_y, early_z, early_margin, tap_margin, lit_taps, clamped)"""
    H, W = smap.shape
    px, py, pz = lp[0] / lp[3], lp[1] / lp[3], lp[2] / lp[3]
    px, py, pz = px * T(0.5) + T(0.5), py * T(0.5) + T(0.5), pz * T(0.5) + T(0.5)
    py = T(1) - py
    early_x, early_y, early_z = (px > 1) | (px < 0), (py > 1) | (py < 0), pz < T(0.5)
    early = early_x | early_y | early_z
    margin = np.minimum.reduce([np.abs(px), np.abs(px - 1), np.abs(py), np.abs(py - 1), np.abs(pz - T(0.5))])
    tsx, tsy = T(1) / T(W), T(1) / T(H)
    current = pz + T(BIAS)
    count = np.zeros(px.shape, T)
    tap_margin = np.full(px.shape, np.inf)
    clamped = np.zeros(px.shape, bool)
    for k in range(16):
        ox, oy = T(POISSON[k, 0]) * T(2) * tsx, T(POISSON[k, 1]) * T(2) * tsy
        s, cl = sample_map(smap, px + ox, py + oy, T)
        d = s * T(0.5) + T(0.5)
        count = count + np.where(current > d, T(1), T(0))
        tap_margin = np.minimum(tap_margin, np.abs(current.astype(f64) - d.astype(f64)))
        clamped |= cl
    shadow = np.where(early, T(1), count / T(16))
    return shadow, dict(early=early, early_x=early_x & ~early_z, early_y=early_y & ~early_z, early_z=early_z, early_margin=margin, tap_margin=tap_margin,
                        lit_taps=count, clamped=clamped & ~early)


def shade(res, instances, verts, light_direction, light_matrix, projection, view, smap, main0, T=f32):
    """the colour pass's resolve over raster()'s owners -> dict(main [H, W, 4] in T, covered, color (the interpolated colour), lighting, shadow and the
    conditioning, each [H, W])"""
    H, W = res["owner"].shape
    main = np.array(main0, f32).reshape(H, W, 4).astype(T)
    fields = dict(color=np.zeros((H, W, 4), T), lighting=np.zeros((H, W), T), shadow=np.zeros((H, W), T), early=np.zeros((H, W), bool),
                  early_x=np.zeros((H, W), bool), early_y=np.zeros((H, W), bool), early_z=np.zeros((H, W), bool), early_margin=np.full((H, W), np.inf),
                  tap_margin=np.full((H, W), np.inf), clamped=np.zeros((H, W), bool), lit_taps=np.zeros((H, W), T), dot_negative=np.zeros((H, W), bool),
                  min_is_shadow=np.zeros((H, W), bool), floor_taken=np.zeros((H, W), bool), sel_margin=np.full((H, W), np.inf))
    L, P, V = (np.asarray(a, f32).astype(T) for a in (light_matrix, projection, view))
    d = np.asarray(light_direction, f32).astype(T)
    verts = np.asarray(verts, f32)
    with np.errstate(all="ignore"):
        for order in np.unique(res["owner"]):
            if order == 0:
                continue
            p = res["prims"][int(order) - 1]
            inst = instances[p["inst"]]
            jj, ii = np.nonzero(res["owner"] == order)
            X, Y = p["X"], p["Y"]
            px, py = 256 * ii.astype(np.int64) + 128, 256 * jj.astype(np.int64) + 128
            e = [sr._edge(X[1], Y[1], X[2], Y[2], px, py), sr._edge(X[2], Y[2], X[0], Y[0], px, py), sr._edge(X[0], Y[0], X[1], Y[1], px, py)]
            area = sr._edge(X[0], Y[0], X[1], Y[1], X[2], Y[2])
            if T is f32:
                l = [sr._to_f32(q) / sr._to_f32(area) for q in e]
            else:
                l = [q.astype(T) / T(area) for q in e]
            # the clip w and the varyings of the three set-up vertices; a cut one is aI + (aO - aI) t with the position's t
            m = np.asarray(inst["model"], f32).astype(T)
            ws, av = [], []
            for k, (I, O, tt) in enumerate(p["src"]):
                aI = vertex_varyings(verts[I], inst, T)
                if T is f32:
                    w, t = p["w"][k], tt
                else:
                    cI = _vec(P, *_vec(V, *_vec(m, *verts[I][2:5].astype(T), T(1))))
                    w, t = cI[3], None
                    if tt is not None:
                        cO = _vec(P, *_vec(V, *_vec(m, *verts[O][2:5].astype(T), T(1))))
                        dI, dO = cI[3] - cI[2], cO[3] - cO[2]
                        t = dI / (dI - dO)
                        w = cI[3] + (cO[3] - cI[3]) * t
                ws.append(w)
                av.append(aI if tt is None else aI + (vertex_varyings(verts[O], inst, T) - aI) * t)
            q = [l[k] / ws[k] for k in range(3)]
            s = (q[0] + q[1]) + q[2]
            b = [q[k] / s for k in range(3)]
            a = [(av[0][c] * b[0] + av[1][c] * b[1]) + av[2][c] * b[2] for c in range(10)]
            nlen = np.sqrt(dot3(a[7], a[8], a[9], a[7], a[8], a[9]))
            nx, ny, nz = a[7] / nlen, a[8] / nlen, a[9] / nlen
            raw = dot3(-d[0], -d[1], -d[2], nx, ny, nz)
            lighting = np.where(T(0) < raw, raw, T(0))
            shadow, cond = shadow_pcf(smap, _vec(L, a[0], a[1], a[2], T(1)), T)
            mn = np.where(shadow < lighting, shadow, lighting)
            f = np.where(T(0.05) < mn, mn, T(0.05))
            main[jj, ii] = np.stack([a[3] * f, a[4] * f, a[5] * f, a[6]], -1)
            fields["color"][jj, ii] = np.stack(a[3:7], -1)
            fields["lighting"][jj, ii], fields["shadow"][jj, ii] = lighting, shadow
            for k in ("early", "early_x", "early_y", "early_z", "early_margin", "tap_margin", "clamped", "lit_taps"):
                fields[k][jj, ii] = cond[k]
            fields["dot_negative"][jj, ii] = ~(T(0) < raw)
            fields["min_is_shadow"][jj, ii] = shadow < lighting
            fields["floor_taken"][jj, ii] = ~(T(0.05) < mn)
            fields["sel_margin"][jj, ii] = np.minimum.reduce([np.abs(raw), np.abs(shadow - lighting), np.abs(mn - T(0.05))]).astype(f64)
    fields["main"], fields["covered"] = main, res["owner"] != 0
    return fields


def undecided(ref64):
    """covered pixels at which a DISCONTINUOUS decision of the fragment stage is not decided by float64: an early-out or a tap compare within its margin
    (the max / min selections are continuous in their arguments: either branch gives the same value at the threshold)"""
    early_close = ref64["early_margin"] <= EARLY_DECIDED
    taps_close = ~ref64["early"] & (ref64["tap_margin"] <= TAP_DECIDED)
    return ref64["covered"] & (early_close | taps_close)


def allowed_outcomes(ref64):
    """[17 + 1, H, W, 4]: what Main may hold at an undecided pixel -- the float64 colour under every number of lit taps, and under the early-out"""
    l, c = ref64["lighting"], ref64["color"]
    outs = []
    for s in [k / 16.0 for k in range(17)] + [1.0]:
        f = np.maximum(0.05, np.minimum(l, s))
        outs.append(np.concatenate([c[..., :3] * f[..., None], c[..., 3:]], -1))
    return np.stack(outs)


def within(got, want, rel=MAIN_RELATIVE):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    return np.abs(got - want) <= rel * np.abs(want)
