"""What the first version of the multisampled surface pass costs (profiles/msaa/README.md), on surface_cases.boxes_and_ground(256, 1920,
1080) -- 256 boxes (back faces culled) over a ground quad -- with the real shade (six point lights):
  - the two draws through sailor_hip_surface_msaa_draw at 1, 2, 4 and 8 samples against sailor_hip_surface_draw_masked over the same draws (that kernel's code
    object is the parent commit's: tests/test_masked_resources_cpu.py pins it), per kernel, by the context's per-launch device events;
  - the layer read-out, the accumulate and the depth store at 8 samples against the bytes they move and this box's own copy rate (sailor_hip_copy_probe);
  - a whole pass of 8 samples, 8 layers and 4 layers, against the single-sample pass (begin, draws, resolve, shade, composite), by device events round the pass.
2 passes warm up, the medians are of the next 7.  Prints one line a figure and a JSON line at the end.

    python scripts/msaa_timing.py [--out FILE]"""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import surface_cases                                                                                        # noqa: E402
import transparent_cases                                                                                    # noqa: E402
from sailor_amd import _lib, host                                                                           # noqa: E402
from sailor_amd.forward_plus import ForwardPlus, HipContext, SurfacePass, linearize_depth, upload_lights    # noqa: E402
from test_surface_gpu import Uploaded                                                                       # noqa: E402

W, H, BOXES, WARM, TIMED = 1920, 1080, 256, 2, 7


def copy_gbs(ctx, nbytes=512 << 20, launches=20):
    """this box's yardstick, as bench.py takes it: a float4 streaming copy, each launch's own timestamps"""
    src = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device).fill_(1)
    dst = torch.empty_like(src)
    for i in range(3 + launches):
        ctx.time_launches(max(i - 3, 0), 1)
        _lib.check(ctx._lib.sailor_hip_copy_probe(ctx.handle, src.data_ptr(), dst.data_ptr(), nbytes), "sailor_hip_copy_probe", ctx.handle)
        ctx.synchronize()
    return 2 * nbytes / (float(np.median([ctx.timed_launch_ms(i) for i in range(launches)])) * 1e-3) / 1e9


def main():
    ctx = HipContext("cuda:0")
    lib = ctx._lib
    s = surface_cases.boxes_and_ground(BOXES, W, H)
    up = Uploaded(ctx, s)
    frame = host.fill_frame_data(np.eye(4, dtype=np.float32).reshape(16), 90.0, 0.5, 20000.0, W, H)
    frame.view[:] = [float(x) for x in s["view"]]
    frame.projection[:] = [float(x) for x in s["projection"]]
    lights = transparent_cases.lights()
    lights["worldPosition"][:, 1] -= np.float32(150.0)
    d_lights = upload_lights(lights, ctx.device)
    draws = [dict(vertices=v, indices=i, instance_ids=ids, num_drawn=d["num_drawn"], first_instance=d["first_instance"], cull_back=d["cull_back"]) for v, i, ids, d in up.draws]
    sp = SurfacePass(ctx, W, H, max_draws=len(draws))
    target = torch.full((H, W, 4), 0.25, dtype=torch.float32, device=ctx.device)
    results = []

    def report(what, x, bytes_moved=None, box=None):
        med = float(np.median(x))
        extra = "" if bytes_moved is None else f", {bytes_moved / med / 1e6:.0f} GB/s over {bytes_moved / 1e6:.1f} MB ({bytes_moved / med / 1e6 / box:.2f} of the box's copy rate)"
        print(f"{what}: median {med * 1e3:.1f} us (min {min(x) * 1e3:.1f}, max {max(x) * 1e3:.1f}, n={len(x)}){extra}", flush=True)
        results.append(dict(what=what, median_us=med * 1e3, min_us=min(x) * 1e3, max_us=max(x) * 1e3, n=len(x), bytes=bytes_moved))
        return med

    # the single-sample pass: its depth for the light cull, its draws through sailor_hip_surface_draw_masked, and the whole of it
    def single_pass(tgt):
        sp.begin()
        base = 0
        for index, d in enumerate(draws):
            nt = d["indices"].numel() // 3
            desc = _lib.SurfaceDraw(d["vertices"].data_ptr(), d["indices"].data_ptr(), None, nt, d["num_drawn"], base, _lib.SURFACE_CULL_BACK if d["cull_back"] else 0,
                                    d["first_instance"], 0)
            _lib.check(lib.sailor_hip_surface_draw_masked(ctx.handle, C.byref(frame), C.byref(desc), up.instances.data_ptr(), up.materials.data_ptr(), len(s["materials"]),
                                                          up.textures.data_ptr(), up.num_textures, index, W, H, C.byref(sp.band), sp.workspace.data_ptr(),
                                                          sp.workspace.numel()), "sailor_hip_surface_draw_masked", ctx.handle)
            base += host.surface_draw_prims(nt, d["num_drawn"])
        surface, depth, _ = sp.resolve(frame, up.instances, up.materials, up.textures, up.num_textures)
        return depth if tgt is None else sp.composite(shade(surface, None), tgt)
    fp = ForwardPlus(ctx, W, H, len(lights))
    fp.cull(frame, d_lights, len(lights), linearize_depth(ctx, frame, single_pass(None)))
    shade = lambda surface, ao: fp.shade(frame, surface, d_lights, len(lights))
    box = copy_gbs(ctx)
    print(f"the box's copy rate: {box:.0f} GB/s", flush=True)

    def timed(fn, names_wanted, names=None):
        """per-launch medians of the kernels named, and the whole of fn() by device events; names: fn's launches where they are more than the log holds"""
        names = ctx.launches_of(fn) if names is None else (fn(), names)[1]
        ctx.synchronize()
        per, whole = {k: [] for k in names_wanted}, []
        for it in range(WARM + TIMED):
            ctx.time_launches(0, len(names))
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            ctx.synchronize()
            if it < WARM:
                continue
            whole.append(start.elapsed_time(stop))
            for k in names_wanted:
                per[k].append(sum(ctx.timed_launch_ms(i) for i, n in enumerate(names) if n == k))
        return per, whole, names

    per, whole, _ = timed(lambda: single_pass(target), ["k_surface_visibility_masked"])
    base_draw = report("single sample: the draws (sailor_hip_surface_draw_masked, 2 launches)", per["k_surface_visibility_masked"])
    base_pass = report("single sample: the whole pass", whole)
    pixels = W * H
    for S in (1, 2, 4, 8):
        run = lambda L=1, S=S: sp.multisampled(frame, draws, up.instances, up.materials, up.textures, up.num_textures, shade, target, samples=S, layers=L)
        per, _, _ = timed(run, ["k_surface_msaa"])
        t = report(f"{S} samples: the draws (sailor_hip_surface_msaa_draw, 2 launches)", per["k_surface_msaa"])
        print(f"    {t / base_draw:.2f} x the single-sample draws", flush=True)
    S = 8
    run = lambda L: sp.multisampled(frame, draws, up.instances, up.materials, up.textures, up.num_textures, shade, target, samples=S, layers=L)
    one = ctx.launches_of(lambda: run(1))   # begin (2 launches), the two draws, then a layer's launches: read-out, resolve, the shade's, accumulate
    assert one[:5] == ["k_surface_msaa_begin", "k_surface_begin", "k_surface_msaa", "k_surface_msaa", "k_surface_msaa_layer"] and one[-1] == "k_surface_msaa_accumulate", one
    for L in (8, 4):
        per, whole, names = timed(lambda: run(L), ["k_surface_msaa_layer", "k_surface_msaa_accumulate", "k_surface_resolve"], one[:4] + one[4:] * L)
        t = report(f"8 samples, {L} layers: the whole pass ({len(names)} launches)", whole)
        print(f"    {t / base_pass:.2f} x the single-sample pass", flush=True)
        report(f"8 samples, {L} layers: the {L} read-outs together", per["k_surface_msaa_layer"], L * pixels * (S * 8 + 8 + 1) + pixels, box)
        report(f"8 samples, {L} layers: the {L} accumulates together", per["k_surface_msaa_accumulate"])
        report(f"8 samples, {L} layers: the {L} resolves together", per["k_surface_resolve"])
        counts = run(L).cpu().numpy().tolist()
        print(f"    pixels a layer {counts[:-1]}, clipped {counts[-1]}", flush=True)
        results.append(dict(what=f"8 samples, {L} layers: counters", counts=counts))
    # one read-out, one accumulate and the depth store on their own
    per, _, _ = timed(lambda: run(1), ["k_surface_msaa_layer", "k_surface_msaa_accumulate"])
    report("8 samples: one layer read-out", per["k_surface_msaa_layer"], pixels * (S * 8 + 8 + 2), box)
    report("8 samples: one accumulate of a full layer (radiance read, target written)", per["k_surface_msaa_accumulate"], pixels * (16 + 16 + 2), box)
    depth = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
    per, _, _ = timed(lambda: sp.store_sample_depth(depth), ["k_surface_msaa_store_depth"])
    report("8 samples: the depth store (sample depths and the average)", per["k_surface_msaa_store_depth"], pixels * (S * 8 + S * 4 + 4), box)
    line = json.dumps(dict(width=W, height=H, boxes=BOXES, warmup=WARM, timed=TIMED, box_copy_gbs=box, results=results))
    print(line)
    if "--out" in sys.argv:
        Path(sys.argv[sys.argv.index("--out") + 1]).write_text(line + "\n")


if __name__ == "__main__":
    main()
