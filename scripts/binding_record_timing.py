"""Host time of the torch-facing binding per recorded call: N eager ForwardPlus.cull + ForwardPlus.shade recordings on the tiny frame (128 x 96, 512 lights,
prepared lights, the shade from the cull's tile lists: the path as smoke() drives it).  bench.py replays captured graphs in its timed region, so the Python
path is outside it; this is the figure a change to the binding can move.

    python scripts/binding_record_timing.py [--tree DIR] [--records 1000]

--tree: the checkout whose sailor_amd package is timed (default: this one), so that two checkouts can be alternated on one machine by one script.  The
other checkout lies outside this repository and needs its own built sailor_amd/csrc/libsailor_hip.so (its package loads the library from its own tree).
profiles/r12/README.md holds the figures this script gave for the change that introduced HipContext.call.
Prints one JSON line: microseconds per cull + shade pair over the recording loop (the stream is drained before and after, outside the timed region)."""
import argparse
import json
import sys
import time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
ap.add_argument("--records", type=int, default=1000)
args = ap.parse_args()
sys.path.insert(0, args.tree)

import torch  # noqa: E402

import sailor_amd  # noqa: E402
from sailor_amd import synth  # noqa: E402
from sailor_amd.forward_plus import ForwardPlus, HipContext, PreparedLights, upload_lights  # noqa: E402

assert Path(sailor_amd.__file__).resolve().is_relative_to(Path(args.tree).resolve()), sailor_amd.__file__
ctx = HipContext("cuda:0")
f = synth.make_frame("tiny")
W, H, n = f.cam.width, f.cam.height, len(f.lights)
depth, surface = torch.from_numpy(f.depth).to(ctx.device), torch.from_numpy(f.surface).to(ctx.device)
lights = upload_lights(f.lights, ctx.device)
fp = ForwardPlus(ctx, W, H, n, prepared=PreparedLights(ctx, lights, n))
for _ in range(100):   # warm-up: the first launches load the code objects
    fp.cull(f.cam.frame, lights, n, depth)
    fp.shade(f.cam.frame, surface, lights, n)
ctx.synchronize()
t0 = time.perf_counter()
for _ in range(args.records):
    fp.cull(f.cam.frame, lights, n, depth)
    fp.shade(f.cam.frame, surface, lights, n)
t1 = time.perf_counter()
ctx.synchronize()
t2 = time.perf_counter()
print(json.dumps({"tree": args.tree, "records": args.records, "us_per_pair": round((t1 - t0) / args.records * 1e6, 3),
                  "us_per_pair_drained": round((t2 - t0) / args.records * 1e6, 3)}))
