"""Times the three EyeAdaptation kernels (histogram, average, tone map) on one GPU against the box's own copy rate.

usage: eye_adaptation_probe.py [out.json]          the whole probe: every step below as a child process under its own `timeout`, merged into out.json
       eye_adaptation_probe.py --step 4k|8k        one step (prints one JSON line)

A step times, with sailor_hip_context_time_launches (the kernels' own dispatch-packet timestamps), the node's three launches
  * over the C3 radiance (at 8K: the C3 radiance tiled 2 x 2) and over a one-bin constant image -- the LDS-contention worst case,
  * with the radiance freshly written (by the shade at 4K / C3, by a device copy otherwise: 133 MB fit the 256 MB last-level cache), again
    with a cache-flushing copy of 1 GiB in between (which leaves the cache full of the copy's DIRTY lines), and again with a read-only sweep of
    530 MB in between (a histogram of another image: clean lines),
and sailor_hip_copy_probe over the same byte count in the same process.  Figures: median of `REPEATS` runs; bytes moved per second
(histogram: one read; tone map: one read + one write) over the copy's (one read + one write).
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
REPEATS = 15
SIZES = {"4k": (3840, 2160), "8k": (7680, 4320)}
STEP_TIMEOUT_S = 240


def step(which: str) -> dict:
    import numpy as np
    import torch

    from sailor_amd import _lib, synth
    from sailor_amd.forward_plus import EyeAdaptation, ForwardPlus, HipContext, upload_lights

    W, H = SIZES[which]
    ctx = HipContext("cuda:0")
    dev = ctx.device
    f = synth.make_frame("C3")
    fp = ForwardPlus(ctx, f.cam.width, f.cam.height, len(f.lights))
    depth = torch.from_numpy(f.depth).to(dev)
    surface = torch.from_numpy(f.surface).to(dev)
    lights = upload_lights(f.lights, dev)
    fp.cull(f.cam.frame, lights, len(f.lights), depth)
    c3 = fp.shade(f.cam.frame, surface, lights, len(f.lights))
    ctx.synchronize()
    nbytes = W * H * 16
    flush_src = torch.zeros(1 << 28, dtype=torch.float32, device=dev)  # 1 GiB
    flush_dst = torch.empty_like(flush_src)
    out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    ea = EyeAdaptation(ctx, W, H)

    def copy(src, dst, n):
        _lib.check(ctx._lib.sailor_hip_copy_probe(ctx.handle, src.data_ptr(), dst.data_ptr(), n), "sailor_hip_copy_probe", ctx.handle)

    def flush():
        copy(flush_src, flush_dst, flush_src.numel() * 4)

    sweep_image = torch.full((4320, 7680, 4), 0.7, dtype=torch.float32, device=dev)
    sweeper = EyeAdaptation(ctx, 7680, 4320)
    sweep_constants = sweeper.constants(0.0)

    def read_sweep():
        sweeper.histogram(sweep_image, sweep_constants)

    def timed(image, producer, flushed):
        """median microseconds of (histogram, average, tone map) over REPEATS runs of: producer(); [flush();] the node"""
        rows = []
        for _ in range(REPEATS):
            producer()
            if flushed == "flushed":
                flush()
            elif flushed == "read_swept":
                read_sweep()
            ctx.time_launches(0, 3)
            ea.run(image, 1.0 / 60.0, out=out)
            rows.append([ctx.timed_launch_ms(s) * 1e3 for s in range(3)])
        return [statistics.median(r[k] for r in rows) for k in range(3)]

    images = {}
    if which == "4k":
        images["c3"] = (c3, lambda: fp.shade(f.cam.frame, surface, lights, len(f.lights)))  # shade() writes c3's storage again
    else:
        tiled = c3.repeat(2, 2, 1).contiguous()
        staged = tiled.clone()
        images["c3_tiled_2x2"] = (tiled, lambda: copy(staged, tiled, nbytes))
    const = torch.full((H, W, 4), 0.3, dtype=torch.float32, device=dev)
    const_staged = const.clone()
    images["one_bin_constant"] = (const, lambda: copy(const_staged, const, nbytes))

    copy_us = []
    a, b = torch.empty(nbytes // 4, dtype=torch.float32, device=dev), torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
    for _ in range(REPEATS):
        flush()
        ctx.time_launches(0, 1)
        copy(b, a, nbytes)
        copy_us.append(ctx.timed_launch_ms(0) * 1e3)
    copy_med = statistics.median(copy_us)
    copy_rate = 2 * nbytes / (copy_med * 1e-6)
    res = {"size": [W, H], "bytes_per_image": nbytes, "repeats": REPEATS, "copy_probe_us": round(copy_med, 2), "copy_probe_TBps": round(copy_rate / 1e12, 3),
           "device": torch.cuda.get_device_name(0), "runs": {}}
    for name, (image, producer) in images.items():
        for flushed in ("fresh", "flushed", "read_swept"):
            h_us, a_us, t_us = timed(image, producer, flushed)
            res["runs"][f"{name}/{flushed}"] = {
                "histogram_us": round(h_us, 2), "average_us": round(a_us, 2), "tonemap_us": round(t_us, 2), "three_launches_us": round(h_us + a_us + t_us, 2),
                "histogram_TBps": round(nbytes / (h_us * 1e-6) / 1e12, 3), "tonemap_TBps": round(2 * nbytes / (t_us * 1e-6) / 1e12, 3),
                "histogram_over_copy_rate": round(nbytes / (h_us * 1e-6) / copy_rate, 3), "tonemap_over_copy_rate": round(2 * nbytes / (t_us * 1e-6) / copy_rate, 3)}
    ctx.synchronize()
    assert np.isfinite(float(ea.views()[1].cpu()[0]))
    return res


def main() -> int:
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print(json.dumps(step(sys.argv[2])))
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07", "eye_adaptation.json")
    merged = {}
    for which in SIZES:  # one child per step, each under its own time limit; nothing more is started after a step that failed
        p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", which], capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(f"step {which} ended with status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}\n")
            return p.returncode
        merged[which] = json.loads(p.stdout.strip().splitlines()[-1])
        print(which, json.dumps(merged[which]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(merged, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
