"""Scratch probe: K4 sweep time for the standard 3-level hierarchy and for the same entities as roots only."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from sailor_amd import synth, host
from sailor_amd.forward_plus import HipContext, EcsSweep
ctx = HipContext("cuda:0")
cam = synth.make_camera(3840, 2160)
planes, _ = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)
for mode in ("standard", "roots"):
    ents = synth.make_entities(1 << 20)
    if mode == "roots":
        ents.parent[:] = 0xFFFFFFFF
        ents.level_offsets = np.array([0, 1 << 20], np.uint32)
    sw = EcsSweep(ctx, ents)
    for _ in range(5): sw.run(planes)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20): sw.run(planes)
    b.record(); torch.cuda.synchronize()
    print(mode, "levels", list(ents.level_offsets), "ms", a.elapsed_time(b) / 20)

# Trace modes at 2^20 entities (the standard hierarchy, 4K camera), one process: the flat float test, the octree mode without and with the
# inserted words (sailor_hip_ecs_sweep_traced on the same buffers, dInserted NULL or not).  The modes take turns batch by batch; a batch is ten
# launches back to back between one pair of events, so the interval over ten is the kernel's time without the event overhead a single launch
# carries (~7 us); the median of 60 batches per mode.
import ctypes as C
from sailor_amd import _lib
ents = synth.make_entities(1 << 20)
sw = EcsSweep(ctx, ents)
inserted = torch.zeros_like(sw.visibility)
pl = np.ascontiguousarray(planes, np.float32).reshape(24)
offs = sw.level_offsets.ctypes.data_as(C.POINTER(C.c_uint32))
traces = {"octree": _lib.SceneTrace(_lib.TRACE_OCTREE_INT_BOXES, 0, None),
          "octree+inserted": _lib.SceneTrace(_lib.TRACE_OCTREE_INT_BOXES, 0, inserted.data_ptr())}

def launch(mode):
    if mode == "flat":
        sw.run(planes)
        return
    _lib.check(ctx._lib.sailor_hip_ecs_sweep_traced(ctx.handle, sw.n, sw.trs.data_ptr(), sw.parent.data_ptr(), offs, len(sw.level_offsets) - 1,
                                                    sw.local_aabb.data_ptr(), pl.ctypes.data_as(C.POINTER(C.c_float)), sw.world.data_ptr(),
                                                    sw.world_aabb.data_ptr(), sw.visibility.data_ptr(), 0, sw.n, C.byref(traces[mode])),
               "sailor_hip_ecs_sweep_traced", ctx.handle)

modes = ("flat", "octree", "octree+inserted")
for m in modes:
    for _ in range(5): launch(m)
torch.cuda.synchronize()
events = {m: [] for m in modes}
for _ in range(60):
    for m in modes:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10): launch(m)
        b.record()
        events[m].append((a, b))
torch.cuda.synchronize()
times = {m: [a.elapsed_time(b) * 100.0 for a, b in ev] for m, ev in events.items()}   # us per launch
flat = float(np.median(times["flat"]))
for m, t in times.items():
    med = float(np.median(t))
    print(f"trace {m:16s} median {med:7.2f} us per launch  (min {min(t):7.2f}, max {max(t):7.2f}; {med - flat:+.2f} us = {100.0 * (med / flat - 1.0):+.1f} % of flat)")
