"""tests/golden/ExperimentalRenderer.renderer as shipped, through the C++ host mirror, with the opt-in node classes (Clear, ShadowPrepass, ExperimentalParticles)
and Debug.shader enabled: every entry of the file has a node class, one frame over tests/particles_cases.py's scene returns status 0, the driver executed a debug
region for every entry in file order, and Main and DepthBuffer equal, bit for bit, what the three C-ABI calls give on the same inputs.  The same file without the
opt-in skips the one entry and leaves the frame as it was.  (The shipped file lists ten frame entries.)"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import particles_cases as cases
import shadow_prepass_cases as sc
from hbao_cases import noise_texels
from particles_run import Device
from sailor_amd import _lib, host
from sailor_amd.forward_plus import upload_textures
from sailor_amd.runtime_binding import Runtime

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EVSM = 2


def frame_entries(text: str):
    return re.findall(r"^- name: (\w+)", text[text.index("\nframe:"):], re.M)


def download(ctx, ptr, shape, dtype=np.float32):
    out = np.zeros(shape, dtype)
    _lib.check(ctx._lib.sailor_hip_buffer_download(ctx.handle, out.ctypes.data, C.c_void_p(ptr), 0, out.nbytes), "buffer_download", ctx.handle)
    return out


def render(ctx, text, opt_in):
    """one frame of the file -> created, skipped, status, regions, Main, DepthBuffer, the lights path's record 0 and matrix 0, the node's instances and map (None
    without the node).  The casters of tests/shadow_prepass_cases.py's scene give the ShadowPrepass entry its cascades: lightsMatrices[0] is the first one's."""
    s, cam, dev = cases.pass_scene(), cases.runtime_camera(), ctx.device
    vertices, indices = torch.from_numpy(s["vertices"]).to(dev), torch.from_numpy(s["indices"].view(np.int32)).to(dev)
    L = sc.layout(False)
    scene_vertices, scene_indices = torch.from_numpy(L.vertices).to(dev), torch.from_numpy(L.indices.view(np.int32)).to(dev)
    inst = L.instances.copy()
    inst["sphereBounds"][:] = (0.0, 0.0, 0.0, np.sqrt(3.0))
    scene_instances, materials = torch.from_numpy(inst.view(np.uint8).copy()).to(dev), torch.from_numpy(L.materials.view(np.uint8).copy()).to(dev)
    textures, num_textures, keep = upload_textures(ctx, L.textures, L.srgb)
    world_aabb = torch.from_numpy(L.world_aabb).to(dev)
    depth_buffer = torch.full((cases.H, cases.W), 0.75, dtype=torch.float32, device=dev)
    back = torch.full((cases.H, cases.W, 4), -3.0, dtype=torch.float32, device=dev)
    noise = torch.from_numpy(np.ascontiguousarray(noise_texels(), np.float32)).to(dev)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(cam)
        for node in ("Clear", "ShadowPrepass") + (("ExperimentalParticles",) if opt_in else ()):
            rt.enable_node(node)
        rt.enable_shader("Shaders/Debug.shader")
        created, skipped, _targets = rt.load_renderer(text)
        rt.set_render_target("DepthBuffer", depth_buffer)
        rt.set_color_target("BackBuffer", back)
        assert rt.set_sampler("g_noiseSampler", noise, noise.shape[1], noise.shape[0]) == 0
        index = rt.add_light(0, EVSM, sc.LIGHT_POSITION, [0.0, -1.0, 0.0], [3.0, 3.0, 3.0], [100.0, 100.0, 100.0])
        rt.set_light_rotation(index, sc.LIGHT_ROTATION)
        rt.tick_lights()
        rt.set_scene(scene_vertices, scene_indices, scene_instances, materials, textures, num_textures, L.batches)
        rt.set_caster_data(world_aabb, L.last_changed_frames, resolutions=(64, 128, 256, 64), trace="flat")
        published = rt.set_particles(7, 2, 1, 1, 1.0, s["records"], vertices, indices, map_extent=(cases.MAP_W, cases.MAP_H), material_instance=3)
        assert published == (0 if opt_in else -1)
        rt.set_time(1.0 / 60.0, float(s["time"]))
        status = rt.process_frame()
        rt.wait_idle()
        torch.cuda.synchronize()
        p, w, h, _levels = rt.render_target("Main")
        assert (w, h) == (cases.W, cases.H)
        out = dict(created=created, skipped=skipped, status=status, regions=rt.last_frame_regions(), main=download(ctx, p, (h, w, 4)), depth=depth_buffer.cpu().numpy(),
                   back=back.cpu().numpy(), instances=None, map=None, light_matrix=rt.lights_matrices()[0].copy(),
                   lights=download(ctx, rt.buffer("light")[0], (1,), host.LIGHT_DTYPE))
        if opt_in:
            inst, count, smap, mw, mh = rt.particles_buffers()
            assert count == 7 and (mw, mh) == (cases.MAP_W, cases.MAP_H)
            out["instances"] = download(ctx, inst, (7 * 112,), np.uint8)
            out["map"] = download(ctx, smap, (mh, mw))
        return out
    finally:
        rt.close()


def test_the_shipped_graph_loads_with_nothing_skipped_and_draws_the_particles(ctx):
    text = (ROOT / "tests" / "golden" / "ExperimentalRenderer.renderer").read_text()
    entries = frame_entries(text)
    assert entries.count("ExperimentalParticles") == 1 and len(entries) == 10
    got = render(ctx, text, True)
    assert got["skipped"] == 0 and got["created"] == len(entries) and got["status"] == 0, (got["created"], got["skipped"], got["status"])
    at = 0
    for entry in entries:   # every entry's region, in file order (the transfer list's regions and the nodes' inner regions lie between them)
        while at < len(got["regions"]) and not got["regions"][at].startswith(entry):
            at += 1
        assert at < len(got["regions"]), (entry, got["regions"])
        at += 1
    assert got["regions"].count("ExperimentalParticles") == 2      # the Dispatch's on the transfer list, the passes' on the graphics list
    # the three C-ABI calls on the same inputs: the two Clear entries leave Main and DepthBuffer at 0 in front of the node
    s, cam = cases.pass_scene(), cases.runtime_camera()
    frame = host.fill_frame_data(cam.world, cam.fov, cam.z_near, cam.z_far, cases.W, cases.H, current_time=float(s["time"]), delta_time=1.0 / 60.0, aspect=cam.aspect)
    s["view"], s["projection"], s["main0"] = np.array(frame.view[:], np.float32), np.array(frame.projection[:], np.float32), np.zeros((cases.H, cases.W, 4), np.float32)
    s["light_matrix"], s["lights"] = got["light_matrix"], got["lights"]        # what the lights path filled: record 0 and the first cascade's matrix
    assert tuple(s["lights"]["direction"][0]) != (0.0, 0.0, 0.0) and np.abs(s["light_matrix"]).sum() > 0
    d = Device(ctx, s)
    d.frame = frame
    for call, name in ((d.update, "update"), (d.shadow, "shadow"), (d.colour, "draw")):
        _lib.check(call(), f"sailor_hip_particles_{name}", ctx.handle)
    ctx.synchronize()
    np.testing.assert_array_equal(got["instances"], d.instances.cpu().numpy())
    np.testing.assert_array_equal(got["map"].view(np.uint32), d.map.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got["main"].view(np.uint32), d.main.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(got["depth"].view(np.uint32), d.depth.cpu().numpy().view(np.uint32))
    covered = got["depth"] != 0
    assert covered.sum() > 150 and (got["main"][covered][:, 3] > 0).all() and (got["main"][~covered] == 0).all()
    assert np.isfinite(got["back"]).all() and (got["back"] != -3.0).any()
    # without the opt-in: one entry skipped, and the frame is what the other nodes leave
    plain = render(ctx, text, False)
    assert plain["skipped"] == 1 and plain["created"] == len(entries) - 1 and plain["status"] == 0
    assert "ExperimentalParticles" not in plain["regions"]
    assert (plain["main"] == 0).all() and (plain["depth"] == 0).all()
