"""A sequential restatement of the Transparent render queue (sailor_amd/csrc/surface_transparent.hip), written from the rules pinned in include/sailor_hip.h
(the Transparent section): depth test against a READ-ONLY depth attachment, no depth write, every surviving fragment of a pixel blended in ascending primitive
order.

It goes primitive after primitive -- draw, instance, triangle, in the order they are issued -- and appends each primitive's fragments to its pixels' lists.
A fragment's planes are taken from the existing surface restatement (tests/gltf_ref.py) run on the sub-scene that holds ONLY that primitive, behind the depth
attachment: the planes the resolve gives "if the fragment owned the pixel" are exactly those, and the restatement's >= test, near-plane cut, fill and discard
are the surface pass's own.  (The two parts the near plane makes of one triangle never share a pixel, so a primitive adds at most one fragment to a pixel;
the part shows in the order.)  Layer k is the k-th entry of every pixel's list.

A scene is gltf_ref's dict; a draw also carries `blend`: "none", "additive" or "alpha"."""
import numpy as np

import gltf_ref
import surface_ref as ref

f32, f64 = np.float32, np.float64
NONE, ADDITIVE, ALPHA = 0, 1, 2
MODES = {"none": NONE, "additive": ADDITIVE, "alpha": ALPHA}


def primitives(scene):
    """(draw index, the sub-scene's draw, its prim_base) for every (draw, instance, triangle) in primitive order"""
    base = int(scene.get("prim_base", 0))
    for k, d in enumerate(scene["draws"]):
        indices = np.asarray(d["indices"], np.uint32).reshape(-1, 3)
        nt, ids, first = len(indices), d.get("instance_ids"), int(d.get("first_instance", 0))
        nd = int(d["num_drawn"]) if d.get("num_drawn") is not None else (len(ids) if ids is not None else len(scene["instances"]) - first)
        for i in range(nd):
            inst = int(ids[i]) if ids is not None else first + i
            for t in range(nt):
                yield k, dict(d, indices=indices[t:t + 1], instance_ids=np.array([inst], np.uint32), num_drawn=1, first_instance=0), base + 2 * (i * nt + t)
        base += 2 * nd * nt


def layers(scene, depth, rows=None, by_depth=False, strict=False, reverse=False, discarded_take_a_layer=False, count=False):
    """-> (list of layers, stats).  A layer: last uint32 [n, W] (orderPlus1 of the layer's fragment, 0: none), covered bool [n, W], planes float32 [3, n, W, 4],
    emissive float32 [n, W, 4], ao_out float32 [n, W], blend uint8 [n, W], z float32 [n, W].  stats (count=True): per_pixel (the list lengths), rejected (fragments
    that exist and fail the depth test), discarded.
    The mutants: by_depth peels far to near instead of by order; strict tests z > depth; reverse blends in descending order; discarded_take_a_layer ignores the
    discard."""
    W, H = scene["W"], scene["H"]
    r0, r1 = rows if rows is not None else (0, H)
    n = r1 - r0
    depth = np.asarray(depth, f32).reshape(H, W)
    frags = []   # (orderPlus1 [n, W] with 0 where the primitive has no fragment, the sub-scene's render, draw index)
    stats = dict(rejected=0, discarded=0)
    for k, d, base in primitives(scene):
        if discarded_take_a_layer:
            d = dict(d, alpha_cutout=False)
        sub = dict(scene, draws=[d], prim_base=base)
        r = gltf_ref.render(sub, prepass=depth, rows=(r0, r1))
        covered = r["covered"].copy()
        if strict:
            covered &= r["depth"] != depth[r0:r1]
        stats["discarded"] += r["stats"]["discarded"]
        if count:
            anywhere = gltf_ref.render(dict(sub, draws=[dict(d, alpha_cutout=False)]), rows=(r0, r1))["covered"]
            behind = gltf_ref.render(dict(sub, draws=[dict(d, alpha_cutout=False)]), prepass=depth, rows=(r0, r1))["covered"]
            stats["rejected"] += int((anywhere & ~behind).sum())
        if covered.any():
            frags.append((np.where(covered, (r["keys"] & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.uint32(0)), r, k))
    if reverse:
        frags = frags[::-1]
    out, taken = [], np.zeros((n, W), np.int64)
    per_pixel = sum((f[0] != 0).astype(np.int64) for f in frags) if frags else np.zeros((n, W), np.int64)
    for level in range(int(per_pixel.max()) if frags else 0):
        L = dict(last=np.zeros((n, W), np.uint32), covered=np.zeros((n, W), bool), planes=np.empty((3, n, W, 4), f32), emissive=np.empty((n, W, 4), f32),
                 ao_out=np.array(frags[0][1]["ao_in"], f32), blend=np.zeros((n, W), np.uint8), z=np.zeros((n, W), f32))
        for q in range(3):
            L["planes"][q] = ref.UNCOVERED[q]
        L["emissive"][:] = gltf_ref.NO_EMISSIVE
        out.append(L)
    if by_depth:
        # the mutant: a pixel's fragments sorted far to near (ascending reversed-Z depth), ties by order
        for jj, ii in np.argwhere(per_pixel > 0):
            mine = sorted((f for f in frags if f[0][jj, ii]), key=lambda f: (float(f[1]["depth"][jj, ii]), int(f[0][jj, ii])))
            for level, f in enumerate(mine):
                _put(out[level], f, scene, (np.array([jj]), np.array([ii])))
    else:
        for f in frags:
            here = f[0] != 0
            for level in np.unique(taken[here]):
                at = np.nonzero(here & (taken == level))
                _put(out[int(level)], f, scene, at)
            taken[here] += 1
    stats["per_pixel"] = per_pixel
    return out, stats


def _put(L, f, scene, at):
    order, r, k = f
    L["last"][at], L["covered"][at], L["z"][at] = order[at], True, r["depth"][at]
    for q in range(3):
        L["planes"][q][at] = r["planes"][q][at]
    L["emissive"][at], L["ao_out"][at] = r["emissive"][at], r["ao_out"][at]
    L["blend"][at] = MODES[scene["draws"][k].get("blend", "none")]


def blend(mode, src, dst, dtype=f32, add_alpha=False):
    """rule 4 on [..., 4] arrays under per-pixel modes, one rounding of `dtype` per written operation: the source products first, then the destination's,
    then the add or the subtract.  add_alpha is the MUTANT that adds in AlphaBlending's alpha channel."""
    src, dst, mode = np.asarray(src, dtype), np.asarray(dst, dtype), np.asarray(mode)[..., None]
    with np.errstate(all="ignore"):
        a = src[..., 3:4]
        k = dtype(1) - a
        rgb = src[..., :3] * a + dst[..., :3] * k
        alpha = a * a + dst[..., 3:4] * k if add_alpha else a * a - dst[..., 3:4] * k
        return np.where(mode == NONE, src, np.where(mode == ADDITIVE, src + dst, np.concatenate([rgb, alpha], -1))).astype(dtype)


def source(radiance, L, dtype=f32, emissive=True):
    """rule 3: (emissive.rgb + radiance.rgb, P0.w)"""
    radiance = np.asarray(radiance, dtype)
    with np.errstate(all="ignore"):
        rgb = L["emissive"][..., :3].astype(dtype) + radiance[..., :3] if emissive else radiance[..., :3]
    return np.concatenate([rgb, L["planes"][0][..., 3:4].astype(dtype)], -1)


def composite(layer_list, shade, target, dtype=f32, emissive=True, add_alpha=False, limit=None):
    """the whole pass: layer after layer, shade(planes [3, n, W, 4], ao_out [n, W]) -> radiance, blended onto a copy of `target` at the layer's pixels"""
    out = np.array(target, dtype)
    for L in layer_list[:limit]:
        src = source(shade(L["planes"], L["ao_out"]), L, dtype, emissive)
        c = L["covered"]
        out[c] = blend(L["blend"][c], src[c], out[c], dtype, add_alpha)
    return out
