"""The plain forms of the C-ABI held to their general entries, on the device.  The torch-facing binding reaches the library through sailor_hip_light_cull_prepared,
sailor_hip_shade_prepared / _tile_lists and sailor_hip_ecs_sweep_traced only; sailor_hip_light_cull, sailor_hip_shade, sailor_hip_shade_ex, sailor_hip_ecs_sweep and
sailor_hip_ecs_sweep_range stay in the header for other callers, so each is called here once beside the general entry with the arguments it is documented to
forward, and the bytes must be equal."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import EcsSweep, ForwardPlus, upload_lights

pytestmark = pytest.mark.gpu


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_plain_cull_and_shade_are_the_prepared_entries_without_prepared_lights(ctx):
    lib = ctx._lib
    f = synth.make_frame("tiny")
    W, H, n = f.cam.width, f.cam.height, len(f.lights)
    frame = f.cam.frame
    lights, depth = upload_lights(f.lights, ctx.device), torch.from_numpy(f.depth).to(ctx.device)
    surface = torch.from_numpy(f.surface).to(ctx.device)
    plain, general = ForwardPlus(ctx, W, H, n), ForwardPlus(ctx, W, H, n)   # (two workspaces, two sets of lists)
    pc = host.push_constants(frame, W, H, n)

    def cull_args(fp):
        return (ctx.handle, C.byref(frame), C.byref(pc), lights.data_ptr(), depth.data_ptr(), fp.grid.data_ptr(), fp.culled.data_ptr(), fp.culled.numel(),
                fp.workspace.data_ptr(), fp.workspace.numel(), C.byref(fp.band), _lib.CULL_DEFAULT)

    _lib.check(lib.sailor_hip_light_cull(*cull_args(plain)), "sailor_hip_light_cull", ctx.handle)
    _lib.check(lib.sailor_hip_light_cull_prepared(*cull_args(general), None, 0), "sailor_hip_light_cull_prepared", ctx.handle)
    ctx.synchronize()
    assert int(plain.culled[0]) > 0, "the frame has lights in its tiles"
    assert same_bytes(plain.grid, general.grid) and same_bytes(plain.culled, general.culled)

    out = [torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device) for _ in range(3)]
    head = (ctx.handle, C.byref(frame), surface.data_ptr(), H * W, lights.data_ptr(), n, plain.grid.data_ptr(), plain.culled.data_ptr(), None)   # (…, csm = NULL)
    band = C.byref(plain.band)
    _lib.check(lib.sailor_hip_shade(*head, out[0].data_ptr(), band), "sailor_hip_shade", ctx.handle)
    _lib.check(lib.sailor_hip_shade_ex(*head, None, out[1].data_ptr(), band, None), "sailor_hip_shade_ex", ctx.handle)
    _lib.check(lib.sailor_hip_shade_prepared(*head, None, out[2].data_ptr(), band, None, None, 0), "sailor_hip_shade_prepared", ctx.handle)
    ctx.synchronize()
    assert float(out[0][..., :3].max()) > 0, "the frame is lit"
    assert same_bytes(out[0], out[1]) and same_bytes(out[0], out[2])


def test_plain_ecs_sweeps_are_the_traced_entry_over_every_entity_without_a_trace(ctx):
    lib = ctx._lib
    # 130 entities in two levels: three visibility words, the last one partial
    ents = synth.make_entities(130)
    roots = int(ents.level_offsets[1])
    parent = ents.parent.copy()
    parent[roots:] %= roots
    ents = dataclasses.replace(ents, parent=parent, level_offsets=np.uint32([0, roots, 130]))
    cam = synth.make_camera(128, 96)
    planes, _ = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)
    planes = np.ascontiguousarray(planes, np.float32).reshape(24)
    sweeps = [EcsSweep(ctx, ents) for _ in range(3)]
    for s in sweeps:
        s.world.fill_(float("nan")), s.world_aabb.fill_(float("nan"))

    def args(s):
        return (ctx.handle, s.n, s.trs.data_ptr(), s.parent.data_ptr(), s.level_offsets.ctypes.data_as(C.POINTER(C.c_uint32)), len(s.level_offsets) - 1,
                s.local_aabb.data_ptr(), planes.ctypes.data_as(C.POINTER(C.c_float)), s.world.data_ptr(), s.world_aabb.data_ptr(), s.visibility.data_ptr())

    _lib.check(lib.sailor_hip_ecs_sweep(*args(sweeps[0])), "sailor_hip_ecs_sweep", ctx.handle)
    _lib.check(lib.sailor_hip_ecs_sweep_range(*args(sweeps[1]), 0, 130), "sailor_hip_ecs_sweep_range", ctx.handle)
    _lib.check(lib.sailor_hip_ecs_sweep_traced(*args(sweeps[2]), 0, 130, None), "sailor_hip_ecs_sweep_traced", ctx.handle)
    ctx.synchronize()
    assert sweeps[0].visibility.numel() == 3 and not bool(torch.isnan(sweeps[0].world).any())
    for s in sweeps[1:]:
        assert same_bytes(sweeps[0].world, s.world) and same_bytes(sweeps[0].world_aabb, s.world_aabb) and same_bytes(sweeps[0].visibility, s.visibility)
