"""Times the 14 launches of the Bloom node (7 downscales, 7 upscales over the 8-level chain of a 4K `Main`) on one GPU against the box's own copy rate.

usage: bloom_probe.py [out.json]                  the whole probe: every step below as a child process under its own `timeout`, merged into out.json
       bloom_probe.py --step c3|hot                one step (prints one JSON line)

A step times, with sailor_hip_context_time_launches (the kernels' own dispatch-packet timestamps), sailor_hip_bloom at 3840 x 2160 with 8 levels, the
shipped parameters and a 1024 x 1024 synthetic dirt texture, over the C3 radiance (`c3`) or over the C3 radiance with saturated bright patches laid over it
so that the thresholded level 1 is not empty (`hot`; the kernels have no data-dependent branch, the step shows that).  Before every run level 0 is restored
by a device copy of the lit frame.  Beside each launch: sailor_hip_copy_probe over the bytes the launch must move, in the same process.  Also: the whole
chain between two stream events without timing slots (launch gaps included).  Figures: median of `REPEATS` runs.

The bytes a launch must move, with the half-used lines of the stride-2 reads counted as read:
  downscale i -> i + 1 : the source rows some tap resolves to (about every second one), whole, + level i + 1 written
  upscale   i -> i - 1 : level i read + level i - 1 read and written (+ the dirt texture at i == 1)
"""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPEATS = 15
W, H, LEVELS = 3840, 2160, 8
DIRT = 1024
STEP_TIMEOUT_S = 300
STEPS = ("c3", "hot")


def bytes_moved(extents, dirt_bytes):
    """{launch name: bytes} for the 14 launches, in launch order"""
    import numpy as np

    from bloom_ref import src_indices
    out = {}
    for i in range(len(extents) - 1):
        (sw, sh), (dw, dh) = extents[i], extents[i + 1]
        rows = np.unique(src_indices(sh, dh))
        rows = rows[(rows >= 0) & (rows < sh)]
        out[f"down{i}to{i + 1}"] = len(rows) * sw * 16 + dw * dh * 16
    for i in range(len(extents) - 1, 0, -1):
        (sw, sh), (dw, dh) = extents[i], extents[i - 1]
        out[f"up{i}to{i - 1}"] = sw * sh * 16 + 2 * dw * dh * 16 + (dirt_bytes if i == 1 else 0)
    return out


def step(which: str) -> dict:
    import numpy as np
    import torch

    from sailor_amd import _lib, host, synth
    from sailor_amd.forward_plus import Bloom, ForwardPlus, HipContext, upload_lights

    ctx = HipContext("cuda:0")
    dev = ctx.device
    f = synth.make_frame("C3")
    assert (f.cam.width, f.cam.height) == (W, H)
    fp = ForwardPlus(ctx, W, H, len(f.lights))
    lights = upload_lights(f.lights, dev)
    fp.cull(f.cam.frame, lights, len(f.lights), torch.from_numpy(f.depth).to(dev))
    lit = fp.shade(f.cam.frame, torch.from_numpy(f.surface).to(dev), lights, len(f.lights)).clone()
    if which == "hot":  # 64 x 64 patches, three in ten saturated blue or red at 40 .. 400
        rng = np.random.default_rng(9)
        cells = (rng.random((H // 64 + 1, W // 64 + 1)) < 0.3)
        tint = np.where(rng.random(cells.shape + (1,)) < 0.5, np.array([0.03, 0.05, 1.0]), np.array([1.0, 0.04, 0.02])) * rng.uniform(40.0, 400.0, cells.shape + (1,))
        patch = torch.from_numpy(np.kron(np.where(cells[..., None], tint, 0.0), np.ones((64, 64, 1)))[:H, :W].astype(np.float32)).to(dev)
        lit[..., :3] += patch
    dirt = torch.from_numpy(np.random.default_rng(7).random((DIRT, DIRT, 4)).astype(np.float32)).to(dev)
    b = Bloom(ctx, W, H, LEVELS, dirt=dirt)
    chain = torch.zeros(b.chain_floats(), dtype=torch.float32, device=dev)
    level0 = b.level(chain, 0)
    moved = bytes_moved(b.extents, DIRT * DIRT * 16)
    names = list(moved)
    assert len(names) == 2 * (LEVELS - 1)

    rows = []
    for _ in range(REPEATS + 2):
        level0.copy_(lit)
        ctx.time_launches(0, len(names))
        b.run(chain)
        rows.append([ctx.timed_launch_ms(s) * 1e3 for s in range(len(names))])
    rows = rows[2:]  # the first runs load the code objects
    us = [statistics.median(r[k] for r in rows) for k in range(len(names))]

    walls = []
    for _ in range(REPEATS + 2):
        level0.copy_(lit)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream())
        b.run(chain)
        e1.record(torch.cuda.current_stream())
        e1.synchronize()
        walls.append(e0.elapsed_time(e1) * 1e3)
    wall_us = statistics.median(walls[2:])

    big = max(moved.values()) // 2 + 64
    src, dst = torch.zeros(big // 4 + 16, dtype=torch.float32, device=dev), torch.empty(big // 4 + 16, dtype=torch.float32, device=dev)
    res = {"extent": [W, H], "levels": LEVELS, "dirt": [DIRT, DIRT], "repeats": REPEATS, "device": torch.cuda.get_device_name(0), "launches": {}}
    for k, name in enumerate(names):
        n = max(moved[name] // 2 // 16 * 16, 16)  # the copy moves 2 n bytes
        t = []
        for _ in range(REPEATS):
            ctx.time_launches(0, 1)
            _lib.check(ctx._lib.sailor_hip_copy_probe(ctx.handle, src.data_ptr(), dst.data_ptr(), n), "sailor_hip_copy_probe", ctx.handle)
            t.append(ctx.timed_launch_ms(0) * 1e3)
        copy_us = statistics.median(t)
        res["launches"][name] = {"us": round(us[k], 2), "bytes_moved": moved[name], "gb_per_s": round(moved[name] / us[k] / 1e3, 1), "copy_probe_us": round(copy_us, 2),
                                 "over_copy_time": round(us[k] / copy_us, 2), "min_us": round(min(r[k] for r in rows), 2), "max_us": round(max(r[k] for r in rows), 2)}
    res["sum_of_launches_us"] = round(sum(us), 2)
    res["level0_launches_us"] = round(us[0] + us[-1], 2)
    small = [u for n, u in zip(names, us) if min(int(v) for v in re.findall(r"\d+", n)) >= 3]  # both levels 480 x 270 or smaller
    assert len(small) == 8
    res["small_level_launches_us"] = round(sum(small), 2)
    res["whole_chain_between_events_us"] = round(wall_us, 2)
    res["bytes_moved_total"] = sum(moved.values())
    ctx.synchronize()
    level1 = b.level(chain, 1).cpu().numpy()
    out0 = level0.cpu().numpy()
    res["level1_nonzero_share_after_the_chain"] = round(float((level1[..., :3] != 0).any(axis=-1).mean()), 4)
    res["level0_changed_share"] = round(float((out0 != lit.cpu().numpy()).any(axis=-1).mean()), 4)
    assert np.isfinite(out0).all()
    return res


def main() -> int:
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print(json.dumps(step(sys.argv[2])))
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09", "bloom.json")
    merged = {}
    for which in STEPS:  # one child per step, each under its own time limit; nothing more is started after a step that failed
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
