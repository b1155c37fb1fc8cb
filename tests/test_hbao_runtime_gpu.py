"""The HBAO block through the C++ host mirror (GPU): a `.renderer` description of its own with Blit -> PostProcess x 3 -> LinearizeDepth ->
LightCulling -> Environment -> RenderScene, the shipped HBAO parameters (tests/golden/DefaultRenderer.renderer:220-264) and a frame-sized g_AO,
loaded through Runtime.load_renderer.  BlitNode and PostProcessNode record the reference's call sequences against the mirrored RHI; the HIP backend
routes them to sailor_hip_blit_nearest / sailor_hip_hbao / sailor_hip_hbao_blur_pass.  g_AO must equal the fp32 restatement (tests/hbao_ref.py) bit
for bit, and the frame shades with it although no caller supplied an AO plane."""
import numpy as np
import pytest
import torch

import hbao_ref as ref
from hbao_cases import is_lively, noise_texels
from hbao_ref import Ref32
from oracle import oracle
from sailor_amd import synth
from sailor_amd.runtime_binding import Runtime, parse_renderer
from test_runtime_gpu import read_u32

pytestmark = pytest.mark.gpu
f32 = np.float32

HBAO_RENDERER = """---
samplers:
- name: g_noiseSampler
  fileId: ''
  path: Textures/Noise.png

renderTargets:
- name: LinearDepth
  format: R32_SFLOAT
  filtration: Nearest
  width: ViewportWidth
  height: ViewportHeight

- name: HalfDepth
  format: D32_SFLOAT_S8_UINT
  width: ViewportWidth/2
  height: ViewportWidth/2

- name: AO
  format: R8_UNORM
  width: ViewportWidth/2
  height: ViewportWidth/2

- name: TemporaryR8
  format: R8_UNORM
  width: ViewportWidth
  height: ViewportWidth

- name: g_AO   # frame-sized: the shade reads ao at the pixel
  format: R8_UNORM
  width: ViewportWidth
  height: ViewportHeight

frame:
- name: Blit
  renderTargets:
  - src: DepthBuffer
  - dst: HalfDepth

- name: PostProcess
  string:
  - shader: Shaders/HBAO.shader
  - defines: ~
  float:
  - data.occlusionRadius: 700
  - data.occlusionPower: 1.5
  - data.occlusionAttenuation: 0.1
  - data.occlusionBias: 0.05
  - data.noiseScale: 25
  renderTargets:
  - color: AO
  - depthSampler: HalfDepth
  - noiseSampler: g_noiseSampler

- name: PostProcess
  string:
  - shader: Shaders/HBAO_Blur.shader
  - defines: VERTICAL
  float:
  - data.sharpness: 0.5
  - data.distanceScale: 2
  - data.radius: 5
  renderTargets:
  - color: TemporaryR8
  - aoSampler: AO
  - depthSampler: DepthBuffer

- name: PostProcess
  string:
  - shader: Shaders/HBAO_Blur.shader
  - defines: HORIZONTAL
  float:
  - data.sharpness: 0.5
  - data.distanceScale: 2
  - data.radius: 5
  renderTargets:
  - color: g_AO
  - aoSampler: TemporaryR8
  - depthSampler: DepthBuffer

- name: PostProcess   # no entry point for this shader: the node is created and records nothing
  string:
  - shader: Shaders/MotionBlur.shader
  - defines: ~
  renderTargets:
  - color: TemporaryR8
  - colorSampler: AO

- name: LinearizeDepth
  renderTargets:
  - depthStencil: DepthBuffer
  - target: LinearDepth

- name: LightCulling
  renderTargets:
  - depthStencil: LinearDepth

- name: Environment

- name: RenderScene
  string:
  - Tag: Opaque
  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer
"""


def setup(rt, f, raw, sky, with_noise=True):
    W, H = f.cam.width, f.cam.height
    rt.set_camera(f.cam)
    keep = []
    if with_noise:   # published before the graph is built: `noiseSampler: g_noiseSampler` then resolves at build time
        noise = torch.from_numpy(noise_texels()).cuda()
        assert rt.set_sampler("g_noiseSampler", noise, 16, 16) == 0
        keep.append(noise)
    loaded = rt.load_renderer(HBAO_RENDERER)
    rt.set_lights(f.lights)
    d_raw = torch.from_numpy(raw).cuda()
    rt.set_render_target("DepthBuffer", d_raw)
    surface = torch.from_numpy(f.surface).cuda()
    radiance = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rt.set_surface(surface, radiance)
    raw_sky = torch.from_numpy(sky.env_chain).cuda()
    assert rt.set_sky_cubemap(raw_sky, 16, sky.env_levels, irradiance_size=2) == 0   # no ao= : nobody supplies the plane
    keep += [d_raw, surface, raw_sky]
    return loaded, radiance, keep


def test_hbao_block_loaded_from_a_renderer_description():
    n, summary = parse_renderer(HBAO_RENDERER, 128, 96)
    assert n == 9 and summary.count("PostProcess[]") == 4 and "Blit[]{rt src=DepthBuffer;rt dst=HalfDepth;}" in summary
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    zn = f.cam.frame.cameraZNearZFar[0]
    raw = synth.make_raw_depth(f.depth, zn)
    sky = synth.make_ibl_set(W, H, np.zeros((2, 2, 2), np.float32), env_size=16, with_ao=False)
    ext = ((W // 2, W // 2), (W // 2, W // 2), (W, W), (W, H))
    want = Ref32.chain(f.cam.frame, raw, noise_texels(), ref.SHIPPED, ref.SHIPPED_BLUR, *ext)
    assert is_lively(want[1])
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        (created, skipped, targets), radiance, keep = setup(rt, f, raw, sky)
        assert (created, skipped, targets) == (9, 0, 5)   # Blit and PostProcess have node classes: created (the unrouted shader's node too), not skipped
        for _ in range(2):
            assert rt.process_frame() == 0
        rt.wait_idle()
        torch.cuda.synchronize()
        for name, plane in zip(("HalfDepth", "AO", "TemporaryR8", "g_AO"), want):
            p, w, h, levels = rt.render_target(name)
            assert p and (w, h, levels) == (plane.shape[1], plane.shape[0], 1), name
            got = read_u32(p, plane.size * 4).reshape(plane.shape)
            bad = got != plane.view(np.uint32)
            assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} words differ from the restatement"
        lin = oracle.linearize_depth(zn, raw)
        og, oi, _ = oracle.light_cull(f.cam.frame, W, H, f.lights, lin)
        ref_env = oracle.prefilter_env_map(sky.env_chain, 16, sky.env_levels)
        ref_irr = oracle.compute_irradiance_map(ref_env, 16, sky.env_levels, 2)
        lut = oracle.compute_brdf_lut(256, 256)
        oibl, _k = oracle.make_ibl(ref_irr, ref_env, 16, sky.env_levels, lut, want[3])
        want_rad = oracle.shade(f.cam.frame, W, H, f.surface, f.lights, og, oi, ibl=oibl)
        err = np.abs(radiance.cpu().numpy().astype(np.float64) - want_rad)
        assert (err <= 3e-4 * np.abs(want_rad) + 1e-5).all(), err.max()   # the bound of test_runtime_gpu.py's frame-graph test
        no_ao, _k2 = oracle.make_ibl(ref_irr, ref_env, 16, sky.env_levels, lut, None)
        plain = oracle.shade(f.cam.frame, W, H, f.surface, f.lights, og, oi, ibl=no_ao)
        assert (np.abs(plain - want_rad) > 3e-4 * np.abs(want_rad) + 1e-5).mean() > 0.25, "AO = 1 would be a different frame"
    finally:
        rt.close()


def test_a_sampler_published_after_the_graph_was_built_is_found_by_name():
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    raw = synth.make_raw_depth(f.depth, f.cam.frame.cameraZNearZFar[0])
    sky = synth.make_ibl_set(W, H, np.zeros((2, 2, 2), np.float32), env_size=16, with_ao=False)
    want = Ref32.chain(f.cam.frame, raw, noise_texels(), ref.SHIPPED, ref.SHIPPED_BLUR, (W // 2, W // 2), (W // 2, W // 2), (W, W), (W, H))
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        loaded, radiance, keep = setup(rt, f, raw, sky, with_noise=False)
        noise = torch.from_numpy(noise_texels()).cuda()
        assert rt.set_sampler("g_noiseSampler", noise, 16, 16) == 0
        assert rt.process_frame() == 0
        rt.wait_idle()
        torch.cuda.synchronize()
        p, w, h, _l = rt.render_target("g_AO")
        np.testing.assert_array_equal(read_u32(p, W * H * 4).reshape(H, W), want[3].view(np.uint32))
    finally:
        rt.close()


def test_a_missing_noise_sampler_is_refused():
    """`noiseSampler: g_noiseSampler` resolves to nothing: the draw is refused with the invalid-argument status, like a tone-map source of another size"""
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    raw = synth.make_raw_depth(f.depth, f.cam.frame.cameraZNearZFar[0])
    sky = synth.make_ibl_set(W, H, np.zeros((2, 2, 2), np.float32), env_size=16, with_ao=False)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        loaded, radiance, keep = setup(rt, f, raw, sky, with_noise=False)
        assert rt.process_frame() == -1
        rt.wait_idle()
    finally:
        rt.close()
