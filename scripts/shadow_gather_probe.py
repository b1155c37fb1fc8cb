"""Times the shadow pass's instance gather (sailor_hip_shadow_gather_instances_batched) on the benchmark's shadow scene: 1 048 576 entities, the four
cascade masks bench.py's shadow_pass_block computes for them (sweep -> world boxes -> sailor_hip_csm_caster_masks), one job per cascade in one call.

usage: shadow_gather_probe.py [out.json] [entities]

Figures
  kernels     sailor_hip_context_time_launches: the two kernels' own dispatch-packet timestamps, median of REPEATS calls after two warm-up calls
  call        device events around CALLS back-to-back calls, per call
  bytes       algorithmic: 64 B read + 64 B written per selected instance, the mask bits of the four ranges read once, the chunk offsets written and read
  copy rate   the box's own: sailor_hip_copy_probe over a buffer of the same size as the gather's traffic, and torch's copy_ of the same, same timing
  host path   what the parent does instead (bench.py:711-716), once, as context: masks to the host, np.unpackbits / np.nonzero, the id lists uploaded
Reported only: there is no parent kernel to compare against.  Checks the result against NumPy before it times anything.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
REPEATS = 20
CALLS = 200


def main() -> int:
    import numpy as np
    import torch

    from sailor_amd import _lib, host, synth
    from sailor_amd.forward_plus import EcsSweep, HipContext, csm_caster_masks, shadow_gather_instances_batched

    count = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
    ctx = HipContext("cuda:0")
    dev = ctx.device
    cam = synth.make_camera(3840, 2160)
    ents = synth.make_entities(count)
    planes, _ = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)
    world, aabb, _ = EcsSweep(ctx, ents).run(planes)
    sh = synth.make_shadow_set(cam, 16)
    cplanes = np.stack([host.extract_frustum_planes_matrix(sh.lights_matrices[k])[0] for k in range(4)])
    masks = csm_caster_masks(ctx, aabb, cplanes)
    ctx.synchronize()

    rec = np.zeros((count, 24), np.float32)   # the scene's 96-byte PerInstanceData records: the casters' models, a bounding sphere, a material index
    rec[:, :16] = synth.caster_models(world.cpu().numpy(), ents.local_aabb)
    rec[:, 16:20] = 1.0
    rec.view(np.uint32)[:, 20] = np.arange(count, dtype=np.uint32)
    rec_d = torch.from_numpy(rec).to(dev)

    masks_h = masks.cpu().numpy().view(np.uint64)
    ids_h = [np.nonzero(np.unpackbits(masks_h[k].view(np.uint8), bitorder="little")[:count])[0] for k in range(4)]
    outs = [torch.empty((max(len(i), 1), 16), dtype=torch.float32, device=dev) for i in ids_h]
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    jobs = [(masks[k], 0, count, outs[k], counts[k:k + 1]) for k in range(4)]
    ws = shadow_gather_instances_batched(ctx, rec_d, jobs)
    ctx.synchronize()
    assert counts.cpu().tolist() == [len(i) for i in ids_h]
    for k in range(4):
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint32)[: len(ids_h[k])], rec.view(np.uint32)[ids_h[k], :16]), f"cascade {k} differs from NumPy"

    selected = sum(len(i) for i in ids_h)
    chunks = 4 * ((count + 1023) // 1024)
    algo = 128 * selected + 4 * ((count + 7) // 8) + 8 * chunks

    rows = []
    for _ in range(REPEATS + 2):
        ctx.time_launches(0, 2)
        shadow_gather_instances_batched(ctx, rec_d, jobs, ws)
        ctx.synchronize()
        rows.append([ctx.timed_launch_ms(s) * 1e3 for s in range(2)])
    rows = rows[2:]
    scan_us, gather_us = (statistics.median(r[k] for r in rows) for k in range(2))

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        shadow_gather_instances_batched(ctx, rec_d, jobs, ws)
    b.record()
    torch.cuda.synchronize()
    call_us = a.elapsed_time(b) * 1e3 / CALLS

    # the box's copy rate over the same number of bytes (half read, half written)
    half = max(algo // 2 // 16 * 16, 16)
    src = torch.empty(half, dtype=torch.uint8, device=dev)
    dst = torch.empty(half, dtype=torch.uint8, device=dev)
    src.zero_(); dst.zero_()
    probe = []
    for _ in range(REPEATS + 2):
        ctx.time_launches(0, 2)
        _lib.check(ctx._lib.sailor_hip_copy_probe(ctx.handle, src.data_ptr(), dst.data_ptr(), half), "sailor_hip_copy_probe", ctx.handle)
        ctx.synchronize()
        probe.append(ctx.timed_launch_ms(1) * 1e3)
    copy_us = statistics.median(probe[2:])
    dst.copy_(src)
    a.record()
    for _ in range(CALLS):
        dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    torch_copy_us = a.elapsed_time(b) * 1e3 / CALLS

    # the parent's path, once: masks to the host, unpack, upload the id lists
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mh = masks.cpu().numpy().view(np.uint64)
    ids = [np.nonzero(np.unpackbits(mh[k].view(np.uint8), bitorder="little")[:count])[0].astype(np.uint32) for k in range(4)]
    up = [torch.from_numpy(i.view(np.int32)).to(dev) for i in ids]
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    assert sum(u.numel() for u in up) == selected

    res = {"device": torch.cuda.get_device_name(0), "entities": count, "jobs": 4, "selected_per_cascade": [int(len(i)) for i in ids_h],
           "density_per_cascade": [round(len(i) / count, 4) for i in ids_h], "algorithmic_bytes": int(algo), "repeats": REPEATS,
           "k_shadow_gather_scan_us": round(scan_us, 2), "k_shadow_gather_us": round(gather_us, 2), "two_kernels_us": round(scan_us + gather_us, 2),
           "two_kernels_gbs": round(algo / (scan_us + gather_us) / 1e3, 1), "gather_kernel_gbs": round(algo / gather_us / 1e3, 1),
           "call_us_back_to_back": round(call_us, 2), "copy_probe_same_bytes_us": round(copy_us, 2), "copy_probe_gbs": round(2 * half / copy_us / 1e3, 1),
           "torch_copy_same_bytes_us": round(torch_copy_us, 2), "torch_copy_gbs": round(2 * half / torch_copy_us / 1e3, 1),
           "host_unpack_and_upload_us_once": round(host_us, 1)}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
