"""The Sky node with clouds through the C++ host mirror (GPU): the frame of tests/test_sky_runtime_gpu.py with the three cloud textures published through
Runtime.sky_set_cloud_textures and "g_noiseSampler" set.  The node then records "Clouds", the sun behind them, "Compose" and "Blit Clouds"
(SkyNode.cpp:565-731), and the `Sky` target equals the chain of the four entry points bit for bit.  Without the textures, or with cloudsDensity = 0, it
records what it recorded before and the target holds the cloudless bits."""
import numpy as np
import pytest
import torch

import clouds_cases as cc
from sailor_amd import forward_plus as fp
from sailor_amd import host, synth
from sailor_amd.runtime_binding import Runtime
from test_runtime_gpu import read_u32
from test_sky_runtime_gpu import SKY_NODE, TARGETS, frames, target

pytestmark = pytest.mark.gpu
f32 = np.float32
SKY_SIZE, SUN_SIZE = 256, 32   # SkyNode.h:14-15
# (no Environment node: the cube bake and the IBL are test_sky_runtime_gpu.py's subject)
CLOUDS_RENDERER = TARGETS + SKY_NODE + """
- name: Blit
  renderTargets:
  - src: Sky
  - dst: Main
"""
NO_DEPTH_RENDERER = TARGETS + """
- name: Sky
  renderTargets:
  - color: Sky
"""




def setup(rt, f, text, noise=None):
    """test_sky_runtime_gpu.setup with half of the depth buffer's 16 x 16 blocks left undrawn (linear depth +inf: the sky shows through) and g_noiseSampler"""
    W, H = f.cam.width, f.cam.height
    rt.set_camera(f.cam)
    loaded = rt.load_renderer(text)
    rt.set_lights(f.lights)
    d_raw = torch.from_numpy(synth.make_raw_depth(f.depth, f.cam.frame.cameraZNearZFar[0], sky_fraction=0.5)).cuda()
    rt.set_render_target("DepthBuffer", d_raw)
    surface = torch.from_numpy(f.surface).cuda()
    radiance = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rt.set_surface(surface, radiance)
    if noise is not None:
        assert rt.set_sampler("g_noiseSampler", noise, noise.shape[1], noise.shape[0]) == 0
    return loaded, [d_raw, surface, radiance, noise]


def device_textures():
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in cc.textures())


def chain(ctx, f, params, tex, depth, clouds_on):
    """the `Sky` target by the entry points: Sky, [Clouds], Sun, Compose, [Blit Clouds] -> (target bits, clouds plane)"""
    W, H = f.cam.width, f.cam.height
    weather, low, high, noise = tex
    frame = f.cam.frame
    size = max(int(min(W * 0.5, H * 0.5)), 1)   # SkyNode.cpp:381-383
    sky = fp.sky_fill(ctx, frame, params, SKY_SIZE)
    clouds = None
    if clouds_on:
        clouds = fp.sky_clouds(ctx, frame, params, sky, weather, low, high, noise, depth, size, size)
        sun = fp.sky_sun_clouds(ctx, frame, params, clouds, SUN_SIZE)
    else:
        sun = fp.sky_sun(ctx, frame, params, SUN_SIZE)
    out = fp.sky_compose(ctx, frame, params, sky, sun, W, H)
    if clouds_on:
        fp.sky_blit_clouds(ctx, clouds, out, W, H)
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint32), (clouds.cpu().numpy() if clouds_on else None)


def linear_depth(rt, ctx, W, H):
    p, w, h, levels = rt.render_target("LinearDepth")
    assert p and (w, h, levels) == (W, H, 1)
    return torch.from_numpy(read_u32(p, W * H * 4).view(f32).reshape(H, W).copy()).to(ctx.device)


def test_sky_node_with_clouds_through_the_frame_graph(ctx):
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    tex = device_textures()
    params = host.sky_params()   # cloudsDensity 0.3, scatteringSteps 5: the node's defaults
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        (created, skipped, targets), keep = setup(rt, f, CLOUDS_RENDERER, noise=tex[3])
        assert (created, skipped, targets) == (3, 0, 3)
        # before the textures are published: the cloudless frame at the default density
        frames(rt, 1)
        depth = linear_depth(rt, ctx, W, H)
        assert torch.isinf(depth).any() and torch.isfinite(depth).any()
        cloudless, _ = chain(ctx, f, params, tex, depth, clouds_on=False)
        assert np.array_equal(target(rt, "Sky", W, H), cloudless)

        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0
        frames(rt, 2)
        want, clouds = chain(ctx, f, params, tex, depth, clouds_on=True)
        covered = (clouds[..., 3] > 0).mean()
        print(f"clouds plane {clouds.shape[1]} x {clouds.shape[0]}: alpha > 0 on {covered:.2f} of it, max alpha {clouds[..., 3].max():.3f}")
        assert 0.02 < covered and clouds[..., 3].max() > 0.5, "no clouds in view: the comparison would show nothing"
        sky = target(rt, "Sky", W, H)
        assert np.array_equal(sky, want), f"{int((sky != want).sum())} words differ from the chain of the four entry points"
        assert not np.array_equal(sky, cloudless)
        assert np.array_equal(target(rt, "Main", W, H), sky)   # Blit src: Sky dst: Main

        # cloudsDensity = 0: the clear branch (SkyNode.cpp:604-609), the cloudless bits
        assert rt.sky_set_params(host.sky_params(cloudsDensity=0.0)) == 0
        frames(rt, 1)
        assert np.array_equal(target(rt, "Sky", W, H), cloudless)
        assert rt.sky_set_params(params) == 0
        frames(rt, 1)
        assert np.array_equal(target(rt, "Sky", W, H), want)
    finally:
        rt.close()


def other_textures():
    """textures of other sizes and contents than clouds_cases': a 16 x 24 weather map and swapped noise volumes"""
    weather, low, high, _ = cc.textures()
    w2 = weather[::2, ::-1][:, :24]
    return tuple(torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (w2, high, low))


def test_republished_textures_replace_the_bound_ones(ctx):
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    tex = device_textures()
    params = host.sky_params()
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        _, keep = setup(rt, f, CLOUDS_RENDERER, noise=tex[3])
        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0
        frames(rt, 1)
        depth = linear_depth(rt, ctx, W, H)
        first, _ = chain(ctx, f, params, tex, depth, clouds_on=True)
        assert np.array_equal(target(rt, "Sky", W, H), first)
        other = other_textures()
        assert tuple(other[0].shape) == (16, 24, 4) and other[1].shape[0] == 8 and other[2].shape[0] == 16
        assert rt.sky_set_cloud_textures(*other) == 0
        tex[0].fill_(0); tex[1].fill_(0); tex[2].fill_(0)   # the earlier textures are the caller's again: nothing may read them any more
        torch.cuda.synchronize()
        frames(rt, 1)
        second, clouds = chain(ctx, f, params, other + (tex[3],), depth, clouds_on=True)
        assert clouds[..., 3].max() > 0.5 and not np.array_equal(second, first)
        sky = target(rt, "Sky", W, H)
        assert np.array_equal(sky, second), f"{int((sky != second).sum())} words differ from the chain over the republished textures"
    finally:
        rt.close()


def test_noise_sampler_set_after_the_textures_is_picked_up(ctx):
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    tex = device_textures()
    params = host.sky_params()
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        _, keep = setup(rt, f, CLOUDS_RENDERER, noise=None)
        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0
        assert rt.process_frame() == -1   # "Clouds" has no g_noiseSampler yet
        rt.wait_idle()
        assert rt.set_sampler("g_noiseSampler", tex[3], tex[3].shape[1], tex[3].shape[0]) == 0
        rt.process_frame()                # (the driver's status keeps the first failure of its lifetime: the target is what shows the recovery)
        rt.wait_idle()
        torch.cuda.synchronize()
        depth = linear_depth(rt, ctx, W, H)
        want, clouds = chain(ctx, f, params, tex, depth, clouds_on=True)
        assert clouds[..., 3].max() > 0.5
        sky = target(rt, "Sky", W, H)
        assert np.array_equal(sky, want), f"{int((sky != want).sum())} words differ from the chain of the four entry points"
    finally:
        rt.close()


def test_clouds_without_the_noise_sampler_or_the_depth_attachment_fail_the_frame(ctx):
    f = synth.make_frame("tiny")
    tex = device_textures()
    for text in (CLOUDS_RENDERER, NO_DEPTH_RENDERER):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        try:
            _, keep = setup(rt, f, text, noise=tex[3] if text is NO_DEPTH_RENDERER else None)
            assert rt.process_frame() == 0   # cloudless: neither is needed
            assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0
            assert rt.process_frame() == -1  # "Clouds" needs g_noiseSampler (binding 8) and linearDepth (binding 9): a name that resolved to nothing
            rt.wait_idle()
        finally:
            rt.close()


def test_a_graph_without_a_sky_node_takes_no_cloud_textures():
    f = synth.make_frame("tiny")
    tex = device_textures()
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        setup(rt, f, TARGETS)
        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == -1
    finally:
        rt.close()
