"""The two routes of the Transparent queue side by side at 3840 x 2160: full-screen layers, an instance a layer, of 2 triangles and of
100 352 small triangles, 1 and 4 layers, through SurfacePass.transparent with the real shade (six point lights).  Both routes run in this process on this
build, alternating pass by pass; 2 passes of each warm up, the medians are of the next 5.  Per kernel (the context's per-launch device events): the peel draw
and the commit of a layer, the bucket draw (once a pass) and the layer read-out; per pass (device events around the recorded pass): the whole pass.
Before it times a configuration it holds the two routes' targets and counters to each other bit for bit.  Prints one line a figure and a JSON line at the end.

    python scripts/transparent_routes_timing.py [--out FILE]"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import transparent_cases as cases                                                                            # noqa: E402
from sailor_amd import host                                                                                  # noqa: E402
from sailor_amd.forward_plus import ForwardPlus, HipContext, SurfacePass, linearize_depth, upload_lights     # noqa: E402
from test_gltf_gpu import Uploaded                                                                           # noqa: E402
from test_transparent_gpu import _grid_mesh                                                                  # noqa: E402

W, H, WARM, TIMED = 3840, 2160, 2, 5


def main():
    ctx = HipContext("cuda:0")
    cam_s = cases.deep_5(W, H)
    cam, lights = cam_s["cam"], cam_s["lights"]
    depth = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
    d_lights = upload_lights(lights, ctx.device)
    fp = ForwardPlus(ctx, W, H, len(lights))
    fp.cull(cam.frame, d_lights, len(lights), linearize_depth(ctx, cam.frame, depth))
    shade = lambda surface, ao: fp.shade(cam.frame, surface, d_lights, len(lights))
    wall = cases.wall(W, H, 1.0)
    meshes = {"2 triangles": (np.asarray(wall[0], np.float32), np.asarray(wall[1], np.uint32)), "100 352 triangles": _grid_mesh(W, H, 224)}
    results = []
    for label, (v, t) in meshes.items():
        for layers in (1, 4):
            models = [host.transform_matrix([0.0, 150.0 * (1.0 - d), 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [d, d, d, 1.0]) for d in (50.0, 40.0, 80.0, 60.0)[:layers]]
            s = cases.cam_scene(W, H, [cases.blended(cases.draw(v, t), "alpha")], models=models, mats=cases.MATS, inst_materials=[0, 1, 2, 0][:layers])
            up = Uploaded(ctx, s)
            draws = [dict(d, blend="alpha") for d in up.draws]
            sp = SurfacePass(ctx, W, H)
            run = lambda mode, target, n=layers: sp.transparent(cam.frame, draws, up.instances, up.materials, up.textures, up.num_textures, depth, shade, target,
                                                                layers=n, mode=mode)
            # the same bits first
            out = {}
            for mode in ("peel", "buckets"):
                target = torch.full((H, W, 4), 0.25, dtype=torch.float32, device=ctx.device)
                counts = run(mode, target)
                ctx.synchronize()
                out[mode] = (target.view(torch.int32).clone(), counts.cpu().numpy().tolist())
            assert torch.equal(out["peel"][0], out["buckets"][0]) and out["peel"][1] == out["buckets"][1] == [W * H] * layers + [0], (out["peel"][1], out["buckets"][1])
            del out
            # the launches of a pass by name, from a pass of one layer: where each kernel sits
            target = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
            names = {mode: ctx.launches_of(lambda: run(mode, target, 1)) for mode in ("peel", "buckets")}
            per_layer = {"peel": len(names["peel"]) - 3, "buckets": len(names["buckets"]) - 3}   # peel: + the overflow round's three; buckets: begin, draw, + the sentinel's read-out
            assert names["peel"][per_layer["peel"]:] == ["k_surface_begin", "k_surface_peel", "k_surface_peel_commit"], names["peel"]
            assert names["buckets"][:3] == ["k_surface_begin", "k_surface_bucket", "k_surface_bucket_layer"] and names["buckets"][-1] == "k_surface_bucket_layer", names["buckets"]
            slots = {"peel": [(names["peel"].index(k), key) for k, key in (("k_surface_peel", "peel draw"), ("k_surface_peel_commit", "commit"))],
                     "buckets": [(names["buckets"].index("k_surface_bucket_layer") - 2, "layer read-out")]}
            total = {"peel": per_layer["peel"] * layers + 3, "buckets": 2 + per_layer["buckets"] * layers + 1}
            times = {mode: {"whole pass": []} for mode in ("peel", "buckets")}
            for it in range(WARM + TIMED):
                for mode in ("peel", "buckets"):
                    ctx.time_launches(0, total[mode])
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record()
                    counts = run(mode, target)
                    stop.record()
                    ctx.synchronize()
                    if it < WARM:
                        continue
                    times[mode]["whole pass"].append(start.elapsed_time(stop))
                    if mode == "buckets":
                        times[mode].setdefault("bucket draw", []).append(ctx.timed_launch_ms(1))
                    first = 0 if mode == "peel" else 2
                    for k in range(layers):
                        for slot, key in slots[mode]:
                            times[mode].setdefault(key, []).append(ctx.timed_launch_ms(first + per_layer[mode] * k + slot))
            assert counts.cpu().numpy().tolist() == [W * H] * layers + [0]
            for mode in ("peel", "buckets"):
                for key, x in times[mode].items():
                    print(f"[{label}, {layers} layer(s), {mode}] {key}: median {np.median(x) * 1e3:.1f} us (min {min(x) * 1e3:.1f}, max {max(x) * 1e3:.1f}, n={len(x)})", flush=True)
                    results.append(dict(mesh=label, layers=layers, route=mode, what=key, median_us=float(np.median(x)) * 1e3, min_us=min(x) * 1e3, max_us=max(x) * 1e3, n=len(x)))
            del up, sp, target
    line = json.dumps(dict(width=W, height=H, warmup=WARM, timed=TIMED, results=results))
    print(line)
    if "--out" in sys.argv:
        Path(sys.argv[sys.argv.index("--out") + 1]).write_text(line + "\n")


if __name__ == "__main__":
    main()
