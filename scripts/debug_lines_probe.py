"""Launch times of the DebugDraw pass at 3840 x 2160 ("DebugDraw"): k_debug_lines_draw and k_debug_lines_resolve, by their own dispatch-packet
timestamps (sailor_hip_context_time_launches), over two scenes:

  boxes   87 382 boxes of DebugContext::DrawAABB's twelve edges = 1 048 584 segments of a few tens of fragments each (the octree of a 1 M-entity world)
  long    4 096 segments from one edge of the screen to the opposite one (frusta, cascade boxes, AABB edges at 4K: thousands of fragments each)

Every repeat begins the pass again (keys of 0), so each draw issues the same atomics.  Prints one JSON line with median / p10 / p90 in microseconds.
SAILOR_HIP_LIB selects the library: scripts/build_variant.sh lanes -DSAILOR_DEBUG_LINES_WAVE_HANDOVER=0 builds the one that leaves every segment to its lane.

    python scripts/debug_lines_probe.py [repeats]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sailor_amd import _lib  # noqa: E402
from sailor_amd.forward_plus import DebugLinesPass, HipContext  # noqa: E402

W, H = 3840, 2160
IDENT = np.eye(4, dtype=np.float32).reshape(16)
EDGES = [(0, 1), (0, 2), (0, 4), (7, 6), (7, 5), (7, 3), (6, 2), (6, 4), (4, 5), (5, 1), (1, 3), (3, 2)]  # DrawAABB's order; corner = x | y << 1 | z << 2 (0 = min)


def boxes(n, rng):
    """clip-space boxes (identity matrix): centres over the screen, 12 .. 40 pixels wide, depth 0.1 .. 0.9, the far face drawn a little smaller"""
    c = np.stack([rng.uniform(-0.98, 0.98, n), rng.uniform(-0.98, 0.98, n), rng.uniform(0.1, 0.9, n)], -1)
    half = np.stack([rng.uniform(6, 20, n) * 2 / W, rng.uniform(6, 20, n) * 2 / H, np.full(n, 0.01)], -1)
    lo, hi = c - half, c + half
    corner = lambda k: np.stack([(hi if k & 1 else lo)[:, 0], (hi if k & 2 else lo)[:, 1], (hi if k & 4 else lo)[:, 2]], -1)  # noqa: E731
    v = np.zeros((n, 12, 2), _lib.VERTEX_P3C4_DTYPE)
    for e, (a, b) in enumerate(EDGES):
        v["position"][:, e, 0], v["position"][:, e, 1] = corner(a), corner(b)
    v["color"] = rng.uniform(0, 1, (n, 1, 1, 4))
    return v.reshape(-1)


def long_segments(n, rng):
    v = np.zeros((n, 2), _lib.VERTEX_P3C4_DTYPE)
    across = rng.random(n) < 0.5
    t0, t1 = rng.uniform(-0.99, 0.99, n), rng.uniform(-0.99, 0.99, n)
    v["position"][:, 0] = np.stack([np.where(across, -0.999, t0), np.where(across, t0, -0.999), rng.uniform(0.1, 0.9, n)], -1)
    v["position"][:, 1] = np.stack([np.where(across, 0.999, t1), np.where(across, t1, 0.999), rng.uniform(0.1, 0.9, n)], -1)
    v["color"] = rng.uniform(0, 1, (n, 2, 4))
    return v.reshape(-1)


def measure(ctx, vertices, repeats):
    dev = ctx.device
    v = torch.from_numpy(vertices.view(np.uint8).copy()).to(dev)
    dp = DebugLinesPass(ctx, W, H)
    depth, target = torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    rows = []
    for _ in range(repeats + 3):
        depth.zero_()
        dp.begin(depth)
        ctx.time_launches(0, 2)
        dp.draw(IDENT, v)
        dp.resolve(target, depth)
        ctx.synchronize()
        rows.append([ctx.timed_launch_ms(0) * 1e3, ctx.timed_launch_ms(1) * 1e3])
    rows = np.array(rows[3:])  # the first runs load the code objects
    keys = dp.download_keys()
    stat = lambda a: {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(np.percentile(a, 10)), 1), "p90_us": round(float(np.percentile(a, 90)), 1)}  # noqa: E731
    return {"segments": len(vertices) // 2, "owned_pixels": int((keys.astype(np.uint32) != 0).sum()), "k_debug_lines_draw": stat(rows[:, 0]),
            "k_debug_lines_resolve": stat(rows[:, 1])}


def main() -> int:
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    if not torch.cuda.is_available():
        raise RuntimeError("the probe needs a HIP device")
    ctx = HipContext("cuda:0")
    rng = np.random.default_rng(3)
    res = {"extent": [W, H], "repeats": repeats, "device": torch.cuda.get_device_name(0), "library": os.environ.get("SAILOR_HIP_LIB", "default"),
           "boxes": measure(ctx, boxes(87382, rng), repeats), "long": measure(ctx, long_segments(4096, rng), repeats)}
    print(json.dumps(res))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
