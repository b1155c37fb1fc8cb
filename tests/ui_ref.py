"""A float32 NumPy restatement of the RenderImGui pass (sailor_amd/csrc/ui_draw.hip), written from the rules pinned in include/sailor_hip.h ("RenderImGui:
ordered alpha-blended UI triangles"): the vertex fetch, ImGuiUI.shader's vertex stage and the unflipped viewport, the snap, 64-bit edge functions with the
top-left rule, the scissor, affine varyings, the bilinear Repeat fetch and the AlphaBlending equations.

It is LITERALLY SEQUENTIAL in the order that matters: command after command, triangle after triangle, each blended over the whole target before the next one is
looked at (the pixels of one triangle are independent of each other and are done as arrays).  Floating point is NumPy float32, one rounding per operation in the
order the header gives; coverage and scissor are integers.

render(..., twin=True) is the float64 TWIN: every floating-point operation behind the snap in double, from the float32-snapped integer positions.  Coverage and
scissor ownership are the same integers, so they must be equal with no pixel left out; colours differ by rounding, except where a fetch picks other texels (the
tap indices are reported, so a test can leave those pixels out and count them).  render(..., reverse=True) is the MUTANT: each command's triangles blended in
reverse order.

flatten() restates Submodules/ImGuiApi.cpp:118-125 and :197-275 (sailor_host_ui_flatten) over draw data as sailor_amd/host.py describes it.

A scene is a dict: W, H, vertices (records of `VERTEX`), indices (uint32), index_bytes (2 or 4), commands (records of `COMMAND`), scale, translate (float32
pairs), texture (uint8 [h, w, 4] or None), target (the seeded plane [H, W, 4] float32, or None: zeros)."""
import numpy as np

f32, f64 = np.float32, np.float64
VERTEX = np.dtype([("position", "<f4", 2), ("uv", "<f4", 2), ("color", "<u4")])
COMMAND = np.dtype([("firstIndex", "<u4"), ("indexCount", "<u4"), ("vertexOffset", "<i4"), ("scissor", "<i4", 4)])
BIN, CHUNK = 32, 256   # UI_BIN, UI_CHUNK of ui_draw.hip: where the cases put their edges and seams
CALLBACK_NONE, CALLBACK_RESET, CALLBACK_USER = 0, 1, 2


def trunc_i32(x) -> int:
    """(int32_t) of a float the caller has bounded"""
    return int(np.trunc(f32(x)))


def flatten(draw_data):
    """-> dict(width, height, scale, translate, commands, vertices, indices): ImGui_SetupRenderState's push constants and ImGui_RenderDrawData's loop, fp32"""
    pos, size, fbs = [np.asarray(draw_data[k], f32) for k in ("display_pos", "display_size", "framebuffer_scale")]
    lists = draw_data.get("lists", [])
    with np.errstate(all="ignore"):
        width, height = trunc_i32(size[0] * fbs[0]), trunc_i32(size[1] * fbs[1])            # :198-199
        scale = np.array([f32(2.0) / size[0], f32(2.0) / size[1]], f32)                       # :119-120
        translate = np.array([f32(-1.0) - pos[0] * scale[0], f32(-1.0) - pos[1] * scale[1]], f32)  # :122-123
    out = []
    if width > 0 and height > 0:                                                              # :201-202
        g_vtx = g_idx = 0
        for l in lists:
            for c in l["cmds"]:
                if c.get("callback", CALLBACK_NONE) != CALLBACK_NONE:                         # :224-232: draws nothing
                    continue
                r = np.asarray(c["clip_rect"], f32)
                mn = [(r[0] - pos[0]) * fbs[0], (r[1] - pos[1]) * fbs[1]]                     # :236-237
                mx = [(r[2] - pos[0]) * fbs[0], (r[3] - pos[1]) * fbs[1]]
                mn = [f32(0.0) if v < 0 else v for v in mn]                                   # :240-243
                mx = [f32(width) if mx[0] > f32(width) else mx[0], f32(height) if mx[1] > f32(height) else mx[1]]
                if mx[0] <= mn[0] or mx[1] <= mn[1]:                                          # :244-245
                    continue
                if not (mx[0] > mn[0]) or not (mx[1] > mn[1]):                                # a NaN ClipRect: left out (its cast is undefined)
                    continue
                out.append((c.get("idx_offset", 0) + g_idx, c.get("elem_count", 0), c.get("vtx_offset", 0) + g_vtx,
                            [trunc_i32(mn[0]), trunc_i32(mn[1]), trunc_i32(mx[0] - mn[0]), trunc_i32(mx[1] - mn[1])]))   # :250-251: the truncated DIFFERENCE
            g_idx += len(l["indices"])                                                        # :273-274
            g_vtx += len(l["vertices"])
    vertices = np.concatenate([np.asarray(l["vertices"], VERTEX) for l in lists]) if lists else np.zeros(0, VERTEX)
    indices = np.concatenate([np.asarray(l["indices"], np.uint32) for l in lists]) if lists else np.zeros(0, np.uint32)
    return dict(width=width, height=height, scale=scale, translate=translate, commands=np.array(out, COMMAND) if out else np.zeros(0, COMMAND),
                vertices=vertices, indices=indices)


def scene_from(draw_data, texture=None, target=None, index_bytes=2, W=None, H=None):
    """the scene of flatten(draw_data): the target is the framebuffer the reference derives, unless W, H say otherwise"""
    flat = flatten(draw_data)
    return dict(W=W or flat["width"], H=H or flat["height"], vertices=flat["vertices"], indices=flat["indices"], index_bytes=index_bytes, commands=flat["commands"],
                scale=flat["scale"], translate=flat["translate"], texture=texture, target=target)


def floor_div256(a: int) -> int:
    return a // 256


def setup(scene, cmd, k, rows):
    """triangle k of a command -> None (dropped, or nothing left of its box) or dict: the snapped positions as Python ints in drawing order after the winding
    swap, the vertices' colour words and uvs in that order, the pixel box cut to the scissor, the frame and the rows"""
    W, H = scene["W"], scene["H"]
    idx, vb = scene["indices"], scene["vertices"]
    at = int(cmd["firstIndex"]) + 3 * k
    if at + 2 >= len(idx):
        return None
    if scene["index_bytes"] == 2:
        assert int(idx[at:at + 3].max()) < 65536
    v = [int(cmd["vertexOffset"]) + int(idx[at + q]) for q in range(3)]
    if any(q < 0 or q >= len(vb) for q in v):
        return None
    sc, tr = np.asarray(scene["scale"], f32), np.asarray(scene["translate"], f32)
    X, Y = [], []
    with np.errstate(all="ignore"):
        for q in v:
            p = vb[q]["position"]
            nx, ny = p[0] * sc[0] + tr[0], p[1] * sc[1] + tr[1]
            xf, yf = (nx + f32(1.0)) * (f32(W) * f32(0.5)), (ny + f32(1.0)) * (f32(H) * f32(0.5))
            sx, sy = xf * f32(256.0), yf * f32(256.0)
            if not (abs(sx) < f32(1.0e9)) or not (abs(sy) < f32(1.0e9)):
                return None
            X.append(int(np.rint(sx))); Y.append(int(np.rint(sy)))
    area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area2 == 0:
        return None
    order = [0, 1, 2] if area2 > 0 else [0, 2, 1]
    X, Y, v = [X[q] for q in order], [Y[q] for q in order], [v[q] for q in order]
    i0, i1 = floor_div256(min(X) - 128 + 255), floor_div256(max(X) - 128)
    j0, j1 = floor_div256(min(Y) - 128 + 255), floor_div256(max(Y) - 128)
    ox, oy, ex, ey = [int(q) for q in cmd["scissor"]]
    i0, i1 = max(i0, ox, 0), min(i1, min(ox + ex, W) - 1)
    j0, j1 = max(j0, oy, rows[0]), min(j1, min(oy + ey, rows[1]) - 1)
    if i1 < i0 or j1 < j0:
        return None
    return dict(X=X, Y=Y, area=abs(area2), color=[int(vb[q]["color"]) for q in v], uv=[vb[q]["uv"].astype(f32) for q in v], box=(i0, i1, j0, j1), swapped=area2 < 0)


def top_left(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (dy == 0 and dx > 0) or dy < 0


def coverage(t):
    """-> (j, i, e0, e1, e2): the covered pixels of a set-up triangle inside its box and their edge functions (int64, exact)"""
    i0, i1, j0, j1 = t["box"]
    X, Y = t["X"], t["Y"]
    jj, ii = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64), np.arange(i0, i1 + 1, dtype=np.int64), indexing="ij")
    px, py = 256 * ii + 128, 256 * jj + 128
    edge = lambda a, b: (X[b] - X[a]) * (py - Y[a]) - (Y[b] - Y[a]) * (px - X[a])   # noqa: E731
    e = [edge(1, 2), edge(2, 0), edge(0, 1)]
    tl = [top_left(X[1], Y[1], X[2], Y[2]), top_left(X[2], Y[2], X[0], Y[0]), top_left(X[0], Y[0], X[1], Y[1])]
    inside = np.ones(ii.shape, bool)
    for q in range(3):
        inside &= (e[q] > 0) | ((e[q] == 0) & tl[q])
    return jj[inside], ii[inside], e[0][inside], e[1][inside], e[2][inside]


def sat_int(x):
    """float -> int as the device converts: NaN -> 0, saturating at the ends of int32"""
    x = np.asarray(x, f64)
    return np.where(np.isnan(x), 0, np.clip(np.nan_to_num(x, nan=0.0, posinf=2147483647.0, neginf=-2147483648.0), -2147483648.0, 2147483647.0)).astype(np.int64)


def repeat_tap(n, u, ft):
    x = u * ft(n) - ft(0.5)
    fx = np.floor(x)
    i0 = sat_int(fx) % n
    return i0, np.where(i0 + 1 == n, 0, i0 + 1), x - fx


def texture_fetch(tex, u, v, ft):
    """base level, bilinear, Repeat over RGBA8 as UNORM -> ([n, 4], the taps (x0, y0) that identify the four texels)"""
    if tex is None or tex.shape[0] == 0 or tex.shape[1] == 0:
        z = np.zeros(len(u), np.int64)
        return np.zeros((len(u), 4), ft), (z, z)
    h, w = tex.shape[:2]
    x0, x1, ax = repeat_tap(w, u, ft)
    y0, y1, ay = repeat_tap(h, v, ft)
    un = lambda b: b.astype(ft) / ft(255.0)   # noqa: E731
    t00, t10, t01, t11 = un(tex[y0, x0]), un(tex[y0, x1]), un(tex[y1, x0]), un(tex[y1, x1])
    ax, ay = ax[:, None], ay[:, None]
    top = t00 * (ft(1.0) - ax) + t10 * ax
    bot = t01 * (ft(1.0) - ax) + t11 * ax
    return top * (ft(1.0) - ay) + bot * ay, (x0, y0)


def num_triangles(scene) -> int:
    return int((scene["commands"]["indexCount"] // 3).sum())


def render(scene, rows=None, twin=False, reverse=False):
    """-> dict: target [rows, W, 4] (float32, or float64 for the twin); count int [rows, W] (fragments blended per pixel); last int [rows, W] (the running
    index of the last triangle that blended there, -1: none); taps: per blended triangle (running index, jb, i, x0, y0); stats"""
    W, H = scene["W"], scene["H"]
    rows = (0, H) if rows is None else rows
    ft = f64 if twin else f32
    seed = np.zeros((H, W, 4), f32) if scene.get("target") is None else np.asarray(scene["target"], f32)
    target = seed[rows[0]:rows[1]].astype(ft).copy()
    count = np.zeros(target.shape[:2], np.int64)
    last = np.full(target.shape[:2], -1, np.int64)
    taps, stats = [], {}
    tex = scene.get("texture")
    running = 0
    for cmd in scene["commands"]:
        n = int(cmd["indexCount"]) // 3
        ks = range(n - 1, -1, -1) if reverse else range(n)
        for k in ks:
            t = setup(scene, cmd, k, rows)
            if t is None:
                stats["dropped_or_scissored"] = stats.get("dropped_or_scissored", 0) + 1
                continue
            if t["swapped"]:
                stats["swapped"] = stats.get("swapped", 0) + 1
            j, i, e0, e1, e2 = coverage(t)
            if len(j) == 0:
                continue
            with np.errstate(all="ignore"):
                area = ft(t["area"])
                l = [e0.astype(ft) / area, e1.astype(ft) / area, e2.astype(ft) / area]
                mix = lambda a: (ft(a[0]) * l[0] + ft(a[1]) * l[1]) + ft(a[2]) * l[2]   # noqa: E731
                chan = lambda s: [ft((c >> s) & 255) / ft(255.0) for c in t["color"]]      # noqa: E731
                col = np.stack([mix(chan(0)), mix(chan(8)), mix(chan(16)), mix(chan(24))], axis=1)
                u, v = mix([q[0] for q in t["uv"]]), mix([q[1] for q in t["uv"]])
                texel, tap = texture_fetch(tex, u, v, ft)
                src = col * texel
                jb = j - rows[0]
                dst = target[jb, i]
                sa = src[:, 3]
                om = ft(1.0) - sa
                out = np.empty_like(dst)
                out[:, :3] = src[:, :3] * sa[:, None] + dst[:, :3] * om[:, None]
                out[:, 3] = sa * sa - dst[:, 3] * om
                target[jb, i] = out
            count[jb, i] += 1
            last[jb, i] = running + k
            taps.append((running + k, jb, i, tap[0], tap[1]))
            stats["fragments"] = stats.get("fragments", 0) + len(j)
            if (sa == 0).any():
                stats["fragments_with_zero_alpha"] = stats.get("fragments_with_zero_alpha", 0) + int((sa == 0).sum())
        running += n
    return dict(target=target, count=count, last=last, taps=taps, stats=stats, rows=rows)


def same_bits_or_class(a, b):
    """equal bit for bit, or both NaN (a NaN's payload is not pinned)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
