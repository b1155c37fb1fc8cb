"""The end of the Sky node through the C++ host mirror (GPU): the frame of tests/test_clouds_runtime_gpu.py with the star mesh published through
Runtime.sky_set_stars and "Shaders/Stars.shader" / "Shaders/SunShafts.shader" enabled.  The node then records the region "Stars & Clouds" as the reference
does (SkyNode.cpp:692-747): the star points, the clouds blit, the sun shafts, and the `Sky` target equals compose -> stars -> blit -> shafts called at
the C-ABI bit for bit.  Without the opt-in it records what it recorded before; with the shader enabled and no mesh published the star draw is left out."""
import numpy as np
import pytest
import torch

import clouds_cases as cc
import stars_cases as sc
from sailor_amd import forward_plus as fp
from sailor_amd import host, synth
from sailor_amd.runtime_binding import Runtime, star_vertices
from test_clouds_runtime_gpu import CLOUDS_RENDERER, chain, device_textures, linear_depth, setup
from test_sky_runtime_gpu import SKY_NODE, TARGETS, frames, target

pytestmark = pytest.mark.gpu
f32 = np.float32
STARS, SHAFTS = "Shaders/Stars.shader", "Shaders/SunShafts.shader"
# a PostProcess entry that draws SunShafts.shader over the Sky target with no `cloudsSampler` among its samplers
SHAFTS_WITHOUT_CLOUDS = TARGETS + SKY_NODE + """
- name: PostProcess
  string:
  - shader: Shaders/SunShafts.shader
  - defines: ~
  float:
  - data.sunShaftsIntensity: 0.45
  renderTargets:
  - color: Sky
"""


def full_chain(ctx, f, params, tex, depth, clouds_on, stars, shafts):
    """the `Sky` target by the entry points: Sky, [Clouds], Sun, Compose, then "Stars & Clouds": [stars], [Blit Clouds], [shafts]"""
    W, H = f.cam.width, f.cam.height
    weather, low, high, noise = tex
    frame = f.cam.frame
    size = max(int(min(W * 0.5, H * 0.5)), 1)   # SkyNode.cpp:381-383
    sky = fp.sky_fill(ctx, frame, params, 256)
    if clouds_on:
        clouds = fp.sky_clouds(ctx, frame, params, sky, weather, low, high, noise, depth, size, size)
        sun = fp.sky_sun_clouds(ctx, frame, params, clouds, 32)
    else:
        clouds = torch.zeros((size, size, 4), dtype=torch.float32, device=ctx.device)   # the cleared m_pCloudsTexture
        sun = fp.sky_sun(ctx, frame, params, 32)
    out = fp.sky_compose(ctx, frame, params, sky, sun, W, H)
    if stars is not None:
        stars.draw(frame, host.sky_stars_model(list(frame.cameraPosition)[:3]), clouds, out, W, H)
    if clouds_on:
        fp.sky_blit_clouds(ctx, clouds, out, W, H)
    if shafts:
        fp.sky_sun_shafts(ctx, frame, params, clouds, out, W, H)
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint32)


def mesh(ctx):
    positions, colors, _ = sc.fixture_mesh()
    return fp.SkyStars(ctx, positions, colors), torch.from_numpy(star_vertices(positions, colors)).to(ctx.device), len(positions)


def test_stars_clouds_and_shafts_through_the_frame_graph(ctx):
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    tex = device_textures()
    params = host.sky_params()   # cloudsDensity 0.3, sunShaftsIntensity 0.45, sunShaftsDistance 60: the node's defaults
    stars, vertices, count = mesh(ctx)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.enable_shader(STARS), rt.enable_shader(SHAFTS)
        (created, skipped, targets), keep = setup(rt, f, CLOUDS_RENDERER, noise=tex[3])
        assert (created, skipped, targets) == (3, 0, 3)
        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0 and rt.sky_set_stars(vertices, count) == 0
        frames(rt, 2)
        depth = linear_depth(rt, ctx, W, H)
        want = full_chain(ctx, f, params, tex, depth, True, stars, True)
        sky = target(rt, "Sky", W, H)
        assert np.array_equal(sky, want), f"{int((sky != want).sum())} words differ from compose -> stars -> blit -> shafts at the C-ABI"
        plain, _ = chain(ctx, f, params, tex, depth, clouds_on=True)
        no_stars, no_shafts = full_chain(ctx, f, params, tex, depth, True, None, True), full_chain(ctx, f, params, tex, depth, True, stars, False)
        changed = [int((want != other).any(-1).sum()) for other in (plain, no_stars, no_shafts)]
        print(f"{W} x {H}: pixels that differ from the frame without both / without the stars / without the shafts: {changed}")
        assert all(n > 0 for n in changed), "a draw that changes nothing shows nothing"
        assert np.array_equal(target(rt, "Main", W, H), sky)   # Blit src: Sky dst: Main

        # cloudless (cloudsDensity = 0): stars and shafts over the cleared plane, no blit
        assert rt.sky_set_params(host.sky_params(cloudsDensity=0.0)) == 0
        frames(rt, 1)
        want = full_chain(ctx, f, host.sky_params(cloudsDensity=0.0), tex, depth, False, stars, True)
        assert np.array_equal(target(rt, "Sky", W, H), want)
    finally:
        rt.close()


def test_without_the_opt_in_the_target_is_what_it_was(ctx):
    """passes before and after the change but for sky_set_stars itself: a runtime that did not opt in records neither draw, mesh or no mesh"""
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    tex = device_textures()
    params = host.sky_params()
    _, vertices, count = mesh(ctx)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        _, keep = setup(rt, f, CLOUDS_RENDERER, noise=tex[3])
        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0 and rt.sky_set_stars(vertices, count) == 0
        before, _ = rt.launch_log(0)
        frames(rt, 1)
        after, names = rt.launch_log(16)
        assert not {"k_sky_stars_project", "k_sky_stars_blend", "k_sky_sun_shafts"} & set(names)
        depth = linear_depth(rt, ctx, W, H)
        want, _ = chain(ctx, f, params, tex, depth, clouds_on=True)
        assert np.array_equal(target(rt, "Sky", W, H), want)
    finally:
        rt.close()


@pytest.mark.parametrize("enabled", [(STARS,), (STARS, SHAFTS), (SHAFTS,)])
def test_stars_enabled_but_not_published_leave_the_draw_out(ctx, enabled):
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    tex = device_textures()
    params = host.sky_params()
    stars, vertices, count = mesh(ctx)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        for path in enabled:
            rt.enable_shader(path)
        _, keep = setup(rt, f, CLOUDS_RENDERER, noise=tex[3])
        assert rt.sky_set_cloud_textures(tex[0], tex[1], tex[2]) == 0
        frames(rt, 1)
        depth = linear_depth(rt, ctx, W, H)
        want = full_chain(ctx, f, params, tex, depth, True, None, SHAFTS in enabled)
        assert np.array_equal(target(rt, "Sky", W, H), want)
        # published now: the draw appears, if its shader was enabled
        assert rt.sky_set_stars(vertices, count) == 0
        frames(rt, 1)
        want = full_chain(ctx, f, params, tex, depth, True, stars if STARS in enabled else None, SHAFTS in enabled)
        assert np.array_equal(target(rt, "Sky", W, H), want)
    finally:
        rt.close()


def test_shafts_without_a_clouds_binding_fail_the_frame(ctx):
    f = synth.make_frame("tiny")
    for enable in (False, True):
        rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        try:
            if enable:
                rt.enable_shader(SHAFTS)
            _, keep = setup(rt, f, SHAFTS_WITHOUT_CLOUDS)
            # not enabled: the PostProcess entry's shader is "not ready" and records nothing; enabled: its `cloudsSampler` resolves to nothing
            assert rt.process_frame() == (-1 if enable else 0)
            rt.wait_idle()
        finally:
            rt.close()


def test_a_graph_without_a_sky_node_takes_no_stars_and_other_paths_keep_raising(ctx):
    f = synth.make_frame("tiny")
    _, vertices, count = mesh(ctx)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        setup(rt, f, TARGETS)
        assert rt.sky_set_stars(vertices, count) == -1
        with pytest.raises(ValueError):
            rt.enable_shader("Shaders/Sky.shader")
        with pytest.raises(ValueError):
            rt.enable_shader("Shaders/Stars")
    finally:
        rt.close()
