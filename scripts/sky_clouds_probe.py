"""Times the four launches the Sky node adds or changes with clouds (cloud march, sun behind clouds, compose, clouds blit) at the node's 4K sizes.

usage: sky_clouds_probe.py [out.json]

3840 x 2160 target, 1080 x 1080 clouds plane (min(w, h) / 2, SkyNode.cpp:381-383), 256 x 256 sky, 32 x 32 sun, default SkyParams (cloudsDensity 0.3,
scatteringSteps 5), synth.make_camera's level camera 1.5 m over the ground, linearDepth = zFar everywhere (an open sky: every ray marches).  Textures at the
engine's sizes -- 128^3 and 32^3 R8 noise volumes, a 512 x 512 RGBA8 weather map --, seeded noise smoothed with wrap-around like tests/clouds_cases.py's.
Figures: sailor_hip_context_time_launches (the kernels' own dispatch-packet timestamps), median of REPEATS runs after two warm-up runs.  Reported only:
there is no parent to compare against.
"""
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPEATS = 10
W, H = 3840, 2160
KERNELS = ("clouds", "sun_clouds", "compose", "blit_clouds")


def smooth(rng, shape, passes):
    import numpy as np
    a = rng.random(shape, dtype=np.float32)
    for _ in range(passes):
        for ax in range(a.ndim):
            a = (np.roll(a, 1, ax) + a + np.roll(a, -1, ax)) / np.float32(3.0)
    return (a - a.min()) / (a.max() - a.min())


def main() -> int:
    import numpy as np
    import torch

    from hbao_cases import noise_texels
    from sailor_amd import forward_plus as fp
    from sailor_amd import host, synth
    from sailor_amd.forward_plus import HipContext

    ctx = HipContext("cuda:0")
    dev = ctx.device
    rng = np.random.default_rng(7)
    to8 = lambda a: torch.from_numpy(np.ascontiguousarray(np.round(a * 255.0).astype(np.uint8))).to(dev)
    weather = np.stack([smooth(rng, (512, 512), 6) for _ in range(4)], -1)
    weather[..., 2] = 0.35 + 0.65 * weather[..., 2]
    weather[..., 3] = 0.5 + 0.5 * weather[..., 3]
    weather, low, high = to8(weather), to8(smooth(rng, (128, 128, 128), 2) ** 0.5), to8(smooth(rng, (32, 32, 32), 1))
    noise = torch.from_numpy(np.ascontiguousarray(noise_texels(), np.float32)).to(dev)
    frame, params = synth.make_camera(W, H).frame, host.sky_params()
    size = min(W, H) // 2
    depth = torch.full((H, W), float(frame.cameraZNearZFar[1]), dtype=torch.float32, device=dev)
    sky = fp.sky_fill(ctx, frame, params, 256)
    clouds = torch.empty((size, size, 4), dtype=torch.float32, device=dev)
    target = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    rows = []
    for _ in range(REPEATS + 2):
        ctx.time_launches(0, 4)
        fp.sky_clouds(ctx, frame, params, sky, weather, low, high, noise, depth, size, size, out=clouds)
        sun = fp.sky_sun_clouds(ctx, frame, params, clouds, 32)
        fp.sky_compose(ctx, frame, params, sky, sun, W, H, out=target)
        fp.sky_blit_clouds(ctx, clouds, target, W, H)
        ctx.synchronize()
        rows.append([ctx.timed_launch_ms(s) * 1e3 for s in range(4)])
    rows = rows[2:]
    alpha = clouds[..., 3]
    res = {"device": torch.cuda.get_device_name(0), "target": [W, H], "clouds_plane": [size, size], "repeats": REPEATS,
           "alpha_gt_0": round(float((alpha > 0).float().mean()), 4), "alpha_gt_0.95": round(float((alpha > 0.95).float().mean()), 4), "launches": {}}
    for k, name in enumerate(KERNELS):
        col = [r[k] for r in rows]
        res["launches"][name] = {"us": round(statistics.median(col), 2), "min_us": round(min(col), 2), "max_us": round(max(col), 2)}
    res["four_launches_us"] = round(sum(v["us"] for v in res["launches"].values()), 2)
    assert bool(torch.isfinite(target).all()) and res["alpha_gt_0"] > 0.05, "the probe's sky has no clouds"
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
