"""Times the kernels of ExperimentalParticles at the size DESIGN.md quotes: 65 536 particles x 4 trace frames (262 144 instanced cubes), a 4096 x 4096 map
and a 3840 x 2160 frame, with the context's own launch timing (sailor_hip_context_time_launches: the command processor's timestamps of each kernel).
Prints the median of --repeat runs per kernel and the update kernel's fraction of the HBM roofline on the bytes it moves (two 80-byte records in, 100
bytes out per instance).

    python scripts/particles_timing.py [--repeat 20] [--hbm-tbps 8.0]
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]

from sailor_amd import _lib, host, synth  # noqa: E402
from sailor_amd.forward_plus import HipContext  # noqa: E402

KERNELS = ["k_particles_update", "k_particles_seed (map)", "k_particles_cast", "k_particles_store_map", "k_particles_seed (frame)", "k_particles_visibility",
           "k_particles_resolve"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=65536)
    ap.add_argument("--trace-frames", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--hbm-tbps", type=float, default=8.0, help="the HBM peak the fraction is taken of (MI355X: 8 TB/s)")
    a = ap.parse_args()
    ctx = HipContext("cuda:0")
    lib, dev = ctx._lib, ctx.device
    rng = np.random.default_rng(1)
    n, tf = a.particles, a.trace_frames
    # a swarm inside the light's box and the camera's view (below): short segments, 2 cm to 6 cm thick
    p1 = np.stack([rng.uniform(-9, 9, a.frames * n), rng.uniform(-8, 2, a.frames * n), rng.uniform(-24, -8, a.frames * n)], 1)
    d = rng.normal(size=(a.frames * n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    records = host.pack_particles(np.ones(a.frames * n), np.full(a.frames * n, 0.02), rng.uniform(0.015, 0.04, a.frames * n), p1, rng.uniform(0, 1, (a.frames * n, 4)),
                                  p1 + d * rng.uniform(0.05, 0.2, (a.frames * n, 1)), rng.uniform(0, 1, (a.frames * n, 4)))
    pc = host.particles_constants(n, a.frames, 30, tf, 0.8)
    verts, indices = synth.face_cube_mesh()
    # the eye at (0, 6, 2) pitched down by atan(9 / 17); the light looks down -y over x in [-10, 10], z in [-25, -5]: clip = (x / 10, -(z + 15) / 10, (y + 10) / 20, 1)
    pitch = -np.arctan2(9.0, 17.0)
    world = np.eye(4)
    world[:3, :3] = [[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]]
    world[:3, 3] = (0.0, 6.0, 2.0)
    view = np.linalg.inv(world).T.reshape(16).astype(np.float32)
    light_matrix = np.zeros(16, np.float32)
    light_matrix[[0, 6, 9, 13, 14, 15]] = (0.1, 0.05, -0.1, -1.5, 0.5, 1.0)
    W, H, MW, MH = 3840, 2160, 4096, 4096
    frame = _lib.UboFrameData()
    frame.currentTime = (a.frames - 0.5) / 30.0     # the last frame of the loop: every trail index in range
    frame.view[:] = [float(x) for x in view]
    frame.projection[:] = [float(x) for x in synth.perspective_reversed_z(W, H, near=1.0, f=2.0)]
    light = np.zeros(1, host.LIGHT_DTYPE)
    light["direction"] = (0.0, -1.0, 0.0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    d_records, d_verts, d_indices, d_light, d_matrix = up(records), up(verts), up(indices), up(light), up(light_matrix)
    d_inst = torch.zeros(pc.numInstances * 112, dtype=torch.uint8, device=dev)
    nbytes = int(lib.sailor_hip_particles_workspace_bytes(MW, MH, W, H))
    ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
    smap = torch.zeros((MH, MW), dtype=torch.float32, device=dev)
    main_t = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    depth = torch.zeros((H, W), dtype=torch.float32, device=dev)
    draw = _lib.ParticlesDraw(dVertices=d_verts.data_ptr(), dIndices=d_indices.data_ptr(), numTriangles=len(indices))

    def run():
        _lib.check(lib.sailor_hip_particles_update(ctx.handle, C.byref(frame), C.byref(pc), d_records.data_ptr(), len(records), d_inst.data_ptr()), "update", ctx.handle)
        _lib.check(lib.sailor_hip_particles_shadow(ctx.handle, C.byref(draw), d_inst.data_ptr(), pc.numInstances, d_matrix.data_ptr(), smap.data_ptr(), MW, MH,
                                                   ws.data_ptr(), nbytes), "shadow", ctx.handle)
        _lib.check(lib.sailor_hip_particles_draw(ctx.handle, C.byref(frame), C.byref(draw), d_inst.data_ptr(), pc.numInstances, d_light.data_ptr(), d_matrix.data_ptr(),
                                                 smap.data_ptr(), MW, MH, main_t.data_ptr(), depth.data_ptr(), W, H, ws.data_ptr(), nbytes), "draw", ctx.handle)

    for _ in range(3):
        depth.zero_()
        run()
    ctx.synchronize()
    times = np.zeros((a.repeat, len(KERNELS)))
    for r in range(a.repeat):
        depth.zero_()
        ctx.synchronize()
        ctx.time_launches(0, len(KERNELS))
        run()
        ctx.synchronize()
        times[r] = [ctx.timed_launch_ms(k) * 1e3 for k in range(len(KERNELS))]
    med = np.median(times, axis=0)
    covered = int((depth != 0).sum().item())
    print(f"{pc.numInstances} instances, map {MW} x {MH} ({int((smap != 0).sum().item())} texels written), frame {W} x {H} ({covered} pixels covered), median of {a.repeat}:")
    for name, t in zip(KERNELS, med):
        print(f"  {name:28s} {t:9.1f} us")
    moved = pc.numInstances * (2 * 80 + 100)
    print(f"  update: {moved / 1e6:.1f} MB moved -> {moved / (med[0] * 1e-6) / 1e12:.2f} TB/s = {100 * moved / (med[0] * 1e-6) / (a.hbm_tbps * 1e12):.1f} % of {a.hbm_tbps} TB/s")


if __name__ == "__main__":
    main()
