"""Times the four launches of the HBAO block (nearest blit, HBAO pass, vertical and horizontal bilateral blur) on one GPU against the box's own copy rate.

usage: hbao_probe.py [out.json]                 the whole probe: every step below as a child process under its own `timeout`, merged into out.json
       hbao_probe.py --step shipped|frame       one step (prints one JSON line)

A step times, with sailor_hip_context_time_launches (the kernels' own dispatch-packet timestamps), sailor_hip_hbao_chain at 4K on the C3 depth with the
shipped parameters: HalfDepth and AO 1920 x 1920, TemporaryR8 3840 x 3840, and g_AO 3840 x 3840 as the shipped file declares it (`shipped`) or
3840 x 2160, the size the shade reads (`frame`).  Beside each launch: sailor_hip_copy_probe over the bytes the launch must move (every input plane read
once, the output written once) in the same process.  Figures: median of `REPEATS` runs.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPEATS = 15
W, H = 3840, 2160
OUT_EXTENT = {"shipped": (W, W), "frame": (W, H)}
STEP_TIMEOUT_S = 240
KERNELS = ("blit_nearest", "hbao", "blur_vertical", "blur_horizontal")


def step(which: str) -> dict:
    import numpy as np
    import torch

    from sailor_amd import _lib, host, synth
    from sailor_amd.forward_plus import Hbao, HipContext

    ctx = HipContext("cuda:0")
    dev = ctx.device
    cam = synth.make_camera(W, H)  # the C3 frame's camera and depth (synth.CONFIGS["C3"]); its lights are not needed
    raw = torch.from_numpy(synth.make_raw_depth(synth.make_linear_depth(W, H), cam.z_near)).to(dev)
    texels = np.load(os.path.join(ROOT, "tests", "golden", "hbao_noise.npy")).astype(np.float64) / 255.0
    lin = np.where(texels <= 0.04045, texels / 12.92, ((texels + 0.055) / 1.055) ** 2.4)
    lin[..., 3] = texels[..., 3]
    noise = torch.from_numpy(np.ascontiguousarray(lin.astype(np.float32))).to(dev)
    extents = ((W // 2, W // 2), (W // 2, W // 2), (W, W), OUT_EXTENT[which])
    hb = Hbao(ctx, W, H, noise, extents=extents)
    plane = lambda e: e[0] * e[1] * 4
    depth_b, half_b, ao_b, temp_b, out_b = W * H * 4, plane(extents[0]), plane(extents[1]), plane(extents[2]), plane(extents[3])
    # what each launch must move: the blit reads one source texel per destination texel; the others read their input planes once
    moved = {"blit_nearest": 2 * half_b, "hbao": half_b + ao_b, "blur_vertical": ao_b + depth_b + temp_b, "blur_horizontal": temp_b + depth_b + out_b}

    rows = []
    for _ in range(REPEATS + 2):
        ctx.time_launches(0, 4)
        hb.run(cam.frame, raw)
        rows.append([ctx.timed_launch_ms(s) * 1e3 for s in range(4)])
    rows = rows[2:]  # the first runs load the code objects
    us = [statistics.median(r[k] for r in rows) for k in range(4)]

    big = max(moved.values()) // 2 + 16
    a, b = torch.empty(big // 4 + 4, dtype=torch.float32, device=dev), torch.zeros(big // 4 + 4, dtype=torch.float32, device=dev)
    res = {"g_ao_extent": list(OUT_EXTENT[which]), "extents": [list(e) for e in extents], "repeats": REPEATS, "device": torch.cuda.get_device_name(0), "launches": {}}
    for k, name in enumerate(KERNELS):
        n = moved[name] // 2 // 16 * 16  # the copy moves 2 n bytes
        t = []
        for _ in range(REPEATS):
            ctx.time_launches(0, 1)
            _lib.check(ctx._lib.sailor_hip_copy_probe(ctx.handle, b.data_ptr(), a.data_ptr(), n), "sailor_hip_copy_probe", ctx.handle)
            t.append(ctx.timed_launch_ms(0) * 1e3)
        copy_us = statistics.median(t)
        res["launches"][name] = {"us": round(us[k], 2), "bytes_moved": moved[name], "copy_probe_us": round(copy_us, 2), "over_copy_time": round(us[k] / copy_us, 2),
                                 "min_us": round(min(r[k] for r in rows), 2), "max_us": round(max(r[k] for r in rows), 2)}
    res["four_launches_us"] = round(sum(us), 2)
    ao_texels = extents[1][0] * extents[1][1]
    res["hbao_ns_per_texel"] = round(us[1] * 1e3 / ao_texels, 4)
    ctx.synchronize()
    g = hb.g_ao.cpu().numpy()
    assert np.isfinite(g).all() and 0.0 <= g.min() and g.max() <= 1.0 and len(np.unique(g)) > 32
    res["g_ao_mean"] = round(float(g.mean()), 4)
    return res


def main() -> int:
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print(json.dumps(step(sys.argv[2])))
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08", "hbao.json")
    merged = {}
    for which in OUT_EXTENT:  # one child per step, each under its own time limit; nothing more is started after a step that failed
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
