"""A float32 NumPy restatement of the DebugDraw pass (sailor_amd/csrc/debug_lines.hip), written from the rules pinned in include/sailor_hip.h ("DebugDraw: the
line-list pass of the Gizmo material"): Gizmo.shader's vertex stage, the clip against five planes, the snap, exact integer coverage per major-axis step, linear
depth, perspective-correct colour, GREATER_OR_EQUAL in primitive order.

It is LITERALLY SEQUENTIAL -- segment after segment, fragment after fragment, a >= test against a depth array, no keys and no maximum; the keys are derived from
the depth and owner arrays at the end.  Floating point is NumPy float32, one rounding per operation in the order the header gives; coverage is Python integers.

Next to the result it reports a float64 TWIN (render(..., twin=True)): the same pass with every floating-point operation behind the snap in double, taking the
float32-snapped integer end points and the float32 clip parameters tIn / tOut as given.  Coverage is the same integers, so coverage and owners must be equal
with no case left out; only z and colour differ, by rounding.  perspective=False is the MUTANT: screen-linear colour (b = t).

A scene is a dict: W, H, vp (16 floats, column-major), vertices (records of `VERTEX`), indices (uint32, two per segment, or None: the identity), prim_base,
depth (the seeded DepthBuffer [H, W] float32, or None: zeros), target (the seeded Main [H, W, 4] float32, or None: zeros)."""
import numpy as np

f32, f64 = np.float32, np.float64
VERTEX = np.dtype([("position", "<f4", 3), ("color", "<f4", 4)])
LANE_FRAGMENTS = 64   # DBGL_LANE_FRAGMENTS: more major-axis steps than this go to the wave
PLANES = ("near", "left", "right", "bottom", "top")   # w - z, w + x, w - x, w + y, w - y


def glsl_mul(m, x, y, z, w):
    """mat4 * vec4, ((c0 x + c1 y) + c2 z) + c3 w, m column-major float32[16]"""
    m = np.asarray(m, f32).reshape(4, 4)
    with np.errstate(all="ignore"):
        return ((m[0] * f32(x) + m[1] * f32(y)) + m[2] * f32(z)) + m[3] * f32(w)


def floor_div256(a: int) -> int:
    return a // 256


def setup(scene, segment: int, rows, stats=None):
    """-> None (no fragment) or the set-up segment: the snapped end points as Python ints, what the attributes need, the range [m0, m0 + n) of major-axis
    pixel coordinates cut to the frame (x-major) or the rows (y-major)"""
    def count(k):
        if stats is not None:
            stats[k] = stats.get(k, 0) + 1
    W, H = scene["W"], scene["H"]
    idx = scene.get("indices")
    ia, ib = (int(idx[2 * segment]), int(idx[2 * segment + 1])) if idx is not None else (2 * segment, 2 * segment + 1)
    va, vb = scene["vertices"][ia], scene["vertices"][ib]
    with np.errstate(all="ignore"):
        A, B = glsl_mul(scene["vp"], *va["position"], 1.0), glsl_mul(scene["vp"], *vb["position"], 1.0)
        t_in, t_out = f32(0.0), f32(1.0)
        for k, name in enumerate(PLANES):
            dA = [A[3] - A[2], A[3] + A[0], A[3] - A[0], A[3] + A[1], A[3] - A[1]][k]
            dB = [B[3] - B[2], B[3] + B[0], B[3] - B[0], B[3] + B[1], B[3] - B[1]][k]
            if dA < 0 and dB < 0:
                count("reject_" + name)
                return None
            if dA < 0:
                t = dA / (dA - dB)
                count("cut_in_" + name)
                if t > t_in:
                    t_in = t
            elif dB < 0:
                t = dA / (dA - dB)
                count("cut_out_" + name)
                if t < t_out:
                    t_out = t
        if t_in > t_out:
            count("reject_t_in_beyond_t_out")
            return None
        P0 = A + (B - A) * t_in if t_in > 0 else A
        P1 = A + (B - A) * t_out if t_out < 1 else B
        if not (P0[3] > 0) or not (P1[3] > 0):
            count("reject_w")
            return None
        X, Y, Z = [], [], []
        for P in (P0, P1):
            nx, ny, nz = P[0] / P[3], P[1] / P[3], P[2] / P[3]
            xf = (nx + f32(1.0)) * (f32(W) * f32(0.5))
            yf = (ny + f32(1.0)) * (f32(H) * f32(-0.5)) + f32(H)
            sx, sy = xf * f32(256.0), yf * f32(256.0)
            if not (abs(sx) < f32(1.0e9)) or not (abs(sy) < f32(1.0e9)):
                count("reject_not_finite")
                return None
            X.append(int(np.rint(sx))); Y.append(int(np.rint(sy))); Z.append(nz)
        ca, cb = va["color"].astype(f32), vb["color"].astype(f32)
        c0 = ca + (cb - ca) * t_in if t_in > 0 else ca
        c1 = ca + (cb - ca) * t_out if t_out < 1 else cb
    dX, dY = X[1] - X[0], Y[1] - Y[0]
    if dX == 0 and dY == 0:
        count("zero_length")
        return None
    x_major = abs(dX) >= abs(dY)
    S0, S1 = (X[0], X[1]) if x_major else (Y[0], Y[1])
    if S1 > S0:
        lo, hi = floor_div256(S0 - 128 + 255), floor_div256(S1 - 128 + 255) - 1
    else:
        lo, hi = floor_div256(S1 - 128) + 1, floor_div256(S0 - 128)
    first, last = (0, W - 1) if x_major else (rows[0], rows[1] - 1)
    lo, hi = max(lo, first), min(hi, last)
    if hi < lo:
        count("empty_range")
        return None
    count("x_major" if x_major else "y_major")
    count("rising" if S1 > S0 else "falling")
    if abs(dX) == abs(dY):
        count("major_axis_tie")
    count("lane_path" if hi - lo + 1 <= LANE_FRAGMENTS else "wave_path")
    return dict(X0=X[0], Y0=Y[0], X1=X[1], Y1=Y[1], z0=Z[0], z1=Z[1], w0=P0[3], w1=P1[3], c0=c0, c1=c1, t_in=t_in, t_out=t_out, A=A, B=B, ca=ca, cb=cb,
                x_major=x_major, m0=lo, n=hi - lo + 1)


def fragments(L, W, rows):
    """every fragment of a set-up segment inside the frame and the rows: -> (i, j, M - S0, dS) as Python integer lists"""
    S0, T0 = (L["X0"], L["Y0"]) if L["x_major"] else (L["Y0"], L["X0"])
    dS, dT = (L["X1"] - L["X0"], L["Y1"] - L["Y0"]) if L["x_major"] else (L["Y1"] - L["Y0"], L["X1"] - L["X0"])
    out = []
    for m in range(L["m0"], L["m0"] + L["n"]):
        M = 256 * m + 128
        minor = (T0 * dS + dT * (M - S0)) // (256 * dS)   # Python's // is the exact floor for either sign of the divisor
        i, j = (m, minor) if L["x_major"] else (minor, m)
        if 0 <= i < W and rows[0] <= j < rows[1]:
            out.append((i, j, M - S0))
    return out, dS


def _attributes(L, num, dS, perspective, twin):
    """z and colour of the fragments whose M - S0 are `num`: float32 in the pinned order, or (twin) the same formulas in double from the float32 clip
    coordinates, the float32 t_in / t_out and the exact integers"""
    with np.errstate(all="ignore"):
        if not twin:
            t = np.array([f32(n) for n in num], f32) / f32(dS)
            z = L["z0"] + (L["z1"] - L["z0"]) * t
            if perspective:
                q0, q1 = (f32(1.0) - t) / L["w0"], t / L["w1"]
                b = q1 / (q0 + q1)
            else:
                b = t
            return z.astype(f32), (L["c0"][None, :] + (L["c1"] - L["c0"])[None, :] * b[:, None]).astype(f32)
        A, B, ti, to = L["A"].astype(f64), L["B"].astype(f64), f64(L["t_in"]), f64(L["t_out"])
        P0 = A + (B - A) * ti if ti > 0 else A
        P1 = A + (B - A) * to if to < 1 else B
        ca, cb = L["ca"].astype(f64), L["cb"].astype(f64)
        c0 = ca + (cb - ca) * ti if ti > 0 else ca
        c1 = ca + (cb - ca) * to if to < 1 else cb
        t = np.array(num, f64) / f64(dS)
        z = P0[2] / P0[3] + (P1[2] / P1[3] - P0[2] / P0[3]) * t
        if perspective:
            q0, q1 = (1.0 - t) / P0[3], t / P1[3]
            b = q1 / (q0 + q1)
        else:
            b = t
        return z, c0[None, :] + (c1 - c0)[None, :] * b[:, None]


def num_segments(scene) -> int:
    return (len(scene["indices"]) if scene.get("indices") is not None else len(scene["vertices"])) // 2


def render(scene, rows=None, perspective=True, twin=False):
    """-> dict: keys uint64 [rows, W]; target [rows, W, 4] (the band's rows of Main); depth [H, W] (the whole DepthBuffer, written in the rows); owner int
    [rows, W] (segment index or -1); stats.  With twin=True depth and target are float64 and there are no keys."""
    W, H = scene["W"], scene["H"]
    rows = (0, H) if rows is None else rows
    ft = f64 if twin else f32
    seed_depth = np.zeros((H, W), f32) if scene.get("depth") is None else scene["depth"].astype(f32)
    seed_target = np.zeros((H, W, 4), f32) if scene.get("target") is None else scene["target"].astype(f32)
    depth = seed_depth.astype(ft).copy()
    band = depth[rows[0]:rows[1]]                       # the depth test runs on the rows of the band
    target = seed_target[rows[0]:rows[1]].astype(ft).copy()
    owner = np.full((rows[1] - rows[0], W), -1, np.int64)
    colour = {}
    stats = {}
    for s in range(num_segments(scene)):
        L = setup(scene, s, rows, stats)
        if L is None:
            continue
        frags, dS = fragments(L, W, rows)
        stats["fragments_outside"] = stats.get("fragments_outside", 0) + L["n"] - len(frags)
        if not frags:
            continue
        z, c = _attributes(L, [f[2] for f in frags], dS, perspective, twin)
        for k, (i, j, _) in enumerate(frags):
            if not (z[k] > 0 and z[k] <= 1):
                stats["fragments_beyond_depth_range"] = stats.get("fragments_beyond_depth_range", 0) + 1
                continue
            jb = j - rows[0]
            if z[k] >= band[jb, i]:                      # GREATER_OR_EQUAL, in primitive order
                if z[k] == band[jb, i]:
                    stats["won_a_tie_with_a_segment" if owner[jb, i] >= 0 else "won_a_tie_with_the_seed"] = \
                        stats.get("won_a_tie_with_a_segment" if owner[jb, i] >= 0 else "won_a_tie_with_the_seed", 0) + 1
                elif owner[jb, i] >= 0:
                    stats["overwritten"] = stats.get("overwritten", 0) + 1
                band[jb, i] = z[k]
                owner[jb, i] = s
                target[jb, i] = c[k]
                colour[(jb, i)] = c[k]
            else:
                stats["fragments_behind"] = stats.get("fragments_behind", 0) + 1
    out = dict(target=target, depth=depth, owner=owner, stats=stats, rows=rows)
    if not twin:
        low = np.where(owner >= 0, owner + scene.get("prim_base", 0) + 1, 0).astype(np.uint64)
        out["keys"] = (band.astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
    return out


def same_bits_or_class(a, b):
    """equal bit for bit, or both NaN (a NaN's payload is not pinned)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
