"""tests/golden/DefaultRenderer.renderer as shipped, through the C++ host mirror, with the opt-in node classes (Clear, ShadowPrepass, Bloom) and the tail's shaders
(MotionBlur.shader, Debug.shader) enabled: every entry of the file has a node class, one frame at a small viewport over tests/shadow_prepass_cases.py's scene
returns status 0, the driver executed a debug region for every entry in file order, and BackBuffer is finite."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import shadow_prepass_cases as sc
from hbao_cases import noise_texels
from sailor_amd.forward_plus import upload_textures
from sailor_amd.runtime_binding import Runtime

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
EVSM = 2


def frame_entries(text: str):
    frame = text[text.index("\nframe:"):]
    return re.findall(r"^- name: (\w+)", frame, re.M)


def test_the_shipped_graph_loads_with_nothing_skipped_and_renders_a_frame(ctx):
    text = (ROOT / "tests" / "golden" / "DefaultRenderer.renderer").read_text()
    entries = frame_entries(text)
    assert entries.count("Clear") == 2 and entries.count("ShadowPrepass") == 1 and entries.count("Bloom") == 1 and len(entries) == 23
    L, cam = sc.layout(False), sc.camera()
    dev = ctx.device
    vertices, indices = torch.from_numpy(L.vertices).to(dev), torch.from_numpy(L.indices.view(np.int32)).to(dev)
    inst = L.instances.copy()
    inst["sphereBounds"][:] = (0.0, 0.0, 0.0, np.sqrt(3.0))   # model space: the unit cube's, and more than the unit quad's
    instances, materials = torch.from_numpy(inst.view(np.uint8).copy()).to(dev), torch.from_numpy(L.materials.view(np.uint8).copy()).to(dev)
    textures, num_textures, keep = upload_textures(ctx, L.textures, L.srgb)
    world_aabb = torch.from_numpy(L.world_aabb).to(dev)
    depth_buffer = torch.full((sc.H, sc.W), 0.75, dtype=torch.float32, device=dev)
    back = torch.full((sc.H, sc.W, 4), -3.0, dtype=torch.float32, device=dev)
    noise = torch.from_numpy(np.ascontiguousarray(noise_texels(), np.float32)).to(dev)
    dirt = torch.from_numpy(np.random.default_rng(5).uniform(0, 1, (32, 32, 4)).astype(np.float32)).to(dev)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(cam)
        for node in ("Clear", "ShadowPrepass", "Bloom"):
            rt.enable_node(node)
        for shader in ("Shaders/MotionBlur.shader", "Shaders/Debug.shader"):
            rt.enable_shader(shader)
        created, skipped, targets = rt.load_renderer(text)
        assert skipped == 0 and created == len(entries), (created, skipped)
        rt.set_render_target("DepthBuffer", depth_buffer)
        rt.set_color_target("BackBuffer", back)
        assert rt.set_sampler("g_noiseSampler", noise, noise.shape[1], noise.shape[0]) == 0
        assert rt.set_sampler("g_lensDirtSampler", dirt, 32, 32) == 0
        index = rt.add_light(0, EVSM, sc.LIGHT_POSITION, [0.0, -1.0, 0.0], [3.0, 3.0, 3.0], [100.0, 100.0, 100.0])
        rt.set_light_rotation(index, sc.LIGHT_ROTATION)
        rt.tick_lights()
        rt.set_scene(vertices, indices, instances, materials, textures, num_textures, L.batches)
        rt.set_scene_tags(["Opaque", "Masked"], [0, 0])   # a batch for either queue: both DepthPrepass and both RenderScene entries record their pass
        rt.set_caster_data(world_aabb, L.last_changed_frames, resolutions=(64, 128, 256, 64), trace="flat")
        rt.set_time(1.0 / 60.0, 0.0)
        status = rt.process_frame()
        rt.wait_idle()
        torch.cuda.synchronize()
        assert status == 0, status
        regions = rt.last_frame_regions()
        at = 0
        for entry in entries:   # every entry's region, in file order (the transfer list's regions and the nodes' inner regions lie between them)
            while at < len(regions) and not regions[at].startswith(entry):
                at += 1
            assert at < len(regions), (entry, regions)
            at += 1
        assert len(rt.shadow_passes()) == 4
        assert torch.isfinite(back).all() and (back != -3.0).any()
    finally:
        rt.close()
