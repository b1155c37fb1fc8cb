"""The three C-ABI calls of ExperimentalParticles over torch buffers, for tests/test_particles_gpu.py and tests/test_experimental_renderer_gpu.py."""
import ctypes as C

import numpy as np
import torch

import particles_cases as cases
from sailor_amd import _lib


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(ctx.device)


def frame_of(time=0.0, view=None, projection=None, width=0, height=0):
    f = _lib.UboFrameData()
    f.currentTime = float(time)
    if view is not None:
        f.view[:] = [float(x) for x in view]
        f.projection[:] = [float(x) for x in projection]
        f.viewportSize[:] = [width, height]
    return f


class Device:
    """a pass scene's buffers on the device: mesh, lights, matrices, map, workspace, Main and DepthBuffer"""

    def __init__(self, ctx, s, map_w=cases.MAP_W, map_h=cases.MAP_H, w=cases.W, h=cases.H):
        self.ctx, self.s, self.map_w, self.map_h, self.w, self.h = ctx, s, map_w, map_h, w, h
        self.vertices, self.indices = dev(ctx, s["vertices"]), dev(ctx, s["indices"])
        self.draw = _lib.ParticlesDraw(dVertices=self.vertices.data_ptr(), dIndices=self.indices.data_ptr(), numTriangles=len(s["indices"]))
        self.lights, self.matrices = dev(ctx, s["lights"]), dev(ctx, np.concatenate([s["light_matrix"], np.full(16, np.nan, np.float32)]))
        self.records, self.instances = dev(ctx, s["records"]), dev(ctx, s["before"])
        self.n = int(s["pc"].numInstances)
        self.bytes = int(ctx._lib.sailor_hip_particles_workspace_bytes(map_w, map_h, w, h))
        self.workspace = torch.full((self.bytes // 8,), -1, dtype=torch.int64, device=ctx.device)
        self.map = torch.full((map_h, map_w), -7.0, dtype=torch.float32, device=ctx.device)
        self.main = torch.from_numpy(s["main0"].copy()).to(ctx.device)
        self.depth = torch.zeros((h, w), dtype=torch.float32, device=ctx.device)
        self.frame = frame_of(s["time"], s["view"], s["projection"], w, h)

    def update(self):
        lib = self.ctx._lib
        return lib.sailor_hip_particles_update(self.ctx.handle, C.byref(self.frame), C.byref(self.s["pc"]), self.records.data_ptr(), len(self.s["records"]),
                                               self.instances.data_ptr())

    def shadow(self):
        lib = self.ctx._lib
        return lib.sailor_hip_particles_shadow(self.ctx.handle, C.byref(self.draw), self.instances.data_ptr(), self.n, self.matrices.data_ptr(), self.map.data_ptr(),
                                               self.map_w, self.map_h, self.workspace.data_ptr(), self.bytes)

    def colour(self):
        lib = self.ctx._lib
        return lib.sailor_hip_particles_draw(self.ctx.handle, C.byref(self.frame), C.byref(self.draw), self.instances.data_ptr(), self.n, self.lights.data_ptr(),
                                             self.matrices.data_ptr(), self.map.data_ptr(), self.map_w, self.map_h, self.main.data_ptr(), self.depth.data_ptr(), self.w,
                                             self.h, self.workspace.data_ptr(), self.bytes)

    def download_instances(self):
        return self.instances.cpu().numpy().view(np.dtype(_lib.PARTICLE_INSTANCE_DTYPE)).copy()


def gpu_update(ctx, c):
    """one update case -> the instance buffer afterwards"""
    records, inst = dev(ctx, c["records"]), dev(ctx, c["before"])
    frame = frame_of(c["time"])
    _lib.check(ctx._lib.sailor_hip_particles_update(ctx.handle, C.byref(frame), C.byref(c["pc"]), records.data_ptr(), len(c["records"]), inst.data_ptr()),
               "sailor_hip_particles_update", ctx.handle)
    ctx.synchronize()
    return inst.cpu().numpy().view(np.dtype(_lib.PARTICLE_INSTANCE_DTYPE)).copy()
