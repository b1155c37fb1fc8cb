"""The Bloom node through the C++ host mirror (GPU): `.renderer` texts with Bloom then EyeAdaptation, loaded through Runtime.load_renderer by a
runtime that opted in with Runtime.enable_node("Bloom").  The node records the reference's call sequence (2 (levels - 1) Dispatches over per-level
binding sets); the HIP backend routes them to sailor_hip_bloom_downscale / sailor_hip_bloom_upscale.  Every level of `Main` must equal the fp32
restatement (tests/bloom_ref.py) bit for bit, and the tone-mapped target the eye-adaptation restatement of the BLOOMED frame."""
import numpy as np
import pytest
import torch

import bloom_ref as ref
import eye_adaptation_ref as ea
from bloom_cases import CASES, make_dirt, make_main
from eye_adaptation_ref import Ref32
from sailor_amd import host, synth
from sailor_amd.runtime_binding import Runtime, load, parse_renderer
from test_runtime_gpu import read_u32

pytestmark = pytest.mark.gpu
F = np.float32

HEAD = """---
renderTargets:
- name: LinearDepth
  format: R32_SFLOAT
  filtration: Nearest
  width: ViewportWidth
  height: ViewportHeight

- name: Secondary
  format: R16G16B16A16_SFLOAT
  width: ViewportWidth
  height: ViewportHeight

frame:
"""
RENDER_SCENE = """- name: LinearizeDepth
  renderTargets:
  - depthStencil: DepthBuffer
  - target: LinearDepth

- name: LightCulling
  renderTargets:
  - depthStencil: LinearDepth

- name: RenderScene
  string:
  - Tag: Opaque
  renderTargets:
  - color: Main
  - depthStencil: DepthBuffer

"""
BLOOM_AND_EYE_ADAPTATION = """- name: Bloom
  vec4:
  - bloomIntensity: [%(bloom_intensity)s, 0, 0, 0]
  - dirtIntensity: [%(dirt_intensity)s, 0, 0, 0]
  - threshold: [%(threshold)s, 0, 0, 0]
  - knee: [%(knee)s, 0, 0, 0]
  renderTargets:
  - bloom: Main

- name: EyeAdaptation
  string:
  - toneMappingShader: Shaders/Tonemapping.shader
  - toneMappingDefines: UNCHARTED2 LUMINANCE
  vec4:
  - data.exposure: [1.0, 0, 0, 0]
  - data.whitePoint: [1.4, 1.5, 1.4, 0]
  renderTargets:
  - color: Secondary
  - hdrColor: Main
  - colorSampler: Main
  - depthStencil: DepthBuffer
"""
OPS = ea.UNCHARTED2 | ea.LUMINANCE


def constants_tuple(c):
    return F(c.minLog2Luminance), F(c.invLog2LuminanceRange), F(c.log2LuminanceRange), F(c.numPixels), F(c.timeCoeff)


def main_chain(main, levels):
    """a flat device chain whose level 0 is `main` and whose lower levels hold a value the node must overwrite"""
    h, w = main.shape[:2]
    chain = torch.full((host.mip_chain_texels(w, h, levels) * 4,), -3.0, dtype=torch.float32, device="cuda")
    chain[:w * h * 4].copy_(torch.from_numpy(np.ascontiguousarray(main, F)).reshape(-1).cuda())
    return chain


def check_levels(chain, want, what):
    h, w = want[0].shape[:2]
    for l, (got, wnt) in enumerate(zip(ref.split(chain.cpu().numpy(), w, h, len(want)), want)):
        ok, msg = ref.same_bits(got, wnt)
        assert ok, f"{what}: level {l} of Main: {msg}"


@pytest.mark.parametrize("name", ["c320x200", "odd270x135"])
def test_bloom_then_eye_adaptation_over_a_prepared_main_chain(name):
    c = CASES[name]
    text = HEAD + BLOOM_AND_EYE_ADAPTATION % c.params()
    n, summary = parse_renderer(text, c.width, c.height)
    assert n == 2 and "Bloom[]" in summary and "rt bloom=Main" in summary
    main, dirt = make_main(c), make_dirt()
    want = ref.bloom_chain(main, c.levels, dirt=dirt, **c.params())
    assert not np.array_equal(want[0], main)
    cam = synth.make_camera(c.width, c.height)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(cam)
        assert load().sailor_rt_node_registered(b"Bloom") == 0
        rt.enable_node("Bloom")
        assert load().sailor_rt_node_registered(b"Bloom") == 0        # before, during and after: the class is never in the registry
        d_dirt = torch.from_numpy(dirt).cuda()
        assert rt.set_sampler("g_lensDirtSampler", d_dirt, dirt.shape[1], dirt.shape[0]) == 0
        created, skipped, targets = rt.load_renderer(text)
        assert (created, skipped, targets) == (2, 0, 2)
        chain = main_chain(main, c.levels)
        rt.set_color_target_chain("Main", chain, c.width, c.height, c.levels)
        assert rt.render_target("Main")[1:] == (c.width, c.height, c.levels)
        ldr_ptr, w, h, _ = rt.render_target("Secondary")
        dt = 1.0 / 60.0
        rt.set_time(dt, 0.0)
        assert rt.process_frame() == 0
        rt.wait_idle()
        torch.cuda.synchronize()
        check_levels(chain, want, name)
        # histogram, adapted luminance and tone map are those of the BLOOMED frame
        k = constants_tuple(host.eye_adaptation_constants(c.width, c.height, dt))
        _, want_lum, want_ldr = ea.step(Ref32, want[0], F(0.5), dt, OPS, exposure=1.0, constants=k)
        _, plain_lum, _ = ea.step(Ref32, main, F(0.5), dt, OPS, exposure=1.0, constants=k)
        assert F(want_lum) != F(plain_lum), "the bloom moves the exposure"
        _, lum_ptr = rt.eye_adaptation_state()
        assert read_u32(lum_ptr, 4)[0] == F(want_lum).view(np.uint32)
        got = read_u32(ldr_ptr, w * h * 16).view(F).reshape(h, w, 4)
        assert ea.same_bits_or_class(got, want_ldr).all(), "the LDR target is not the tone map of the bloomed frame"
        assert load().sailor_rt_node_registered(b"Bloom") == 0
    finally:
        rt.close()


def test_without_the_opt_in_the_entry_is_skipped_and_main_untouched():
    c = CASES["c320x200"]
    text = HEAD + BLOOM_AND_EYE_ADAPTATION % c.params()
    main = make_main(c)
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(synth.make_camera(c.width, c.height))
        d_dirt = torch.from_numpy(make_dirt()).cuda()
        rt.set_sampler("g_lensDirtSampler", d_dirt, d_dirt.shape[1], d_dirt.shape[0])
        created, skipped, targets = rt.load_renderer(text)
        assert (created, skipped, targets) == (1, 1, 2)               # "FrameGraph Node Bloom is not implemented!"
        chain = main_chain(main, c.levels)
        before = chain.clone()
        rt.set_color_target_chain("Main", chain, c.width, c.height, c.levels)
        rt.set_time(1.0 / 60.0, 0.0)
        assert rt.process_frame() == 0
        rt.wait_idle()
        torch.cuda.synchronize()
        assert torch.equal(chain.view(torch.int32), before.view(torch.int32))
        with pytest.raises(ValueError):
            rt.enable_node("MotionBlur")                              # no such opt-in class
    finally:
        rt.close()


def test_an_unresolved_lens_dirt_sampler_is_refused():
    """the upscale at mip level 1 samples u_dirt_texture: with no "g_lensDirtSampler" published the Dispatch is refused with the invalid-argument status"""
    c = CASES["pow2_128x96"]
    text = HEAD + BLOOM_AND_EYE_ADAPTATION % c.params()
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(synth.make_camera(c.width, c.height))
        rt.enable_node("Bloom")
        assert rt.load_renderer(text)[:2] == (2, 0)
        chain = main_chain(make_main(c), c.levels)
        rt.set_color_target_chain("Main", chain, c.width, c.height, c.levels)
        rt.set_time(1.0 / 60.0, 0.0)
        assert rt.process_frame() == -1
        rt.wait_idle()
    finally:
        rt.close()


def run_tiny_frame(text, f, raw, levels, opt_in, dirt):
    """the tiny frame through LinearizeDepth -> LightCulling -> RenderScene -> (Bloom) -> EyeAdaptation: (status tuple of load_renderer, the Main chain)"""
    W, H = f.cam.width, f.cam.height
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(f.cam)
        if opt_in:
            rt.enable_node("Bloom")
        d_dirt = torch.from_numpy(dirt).cuda()
        rt.set_sampler("g_lensDirtSampler", d_dirt, dirt.shape[1], dirt.shape[0])
        loaded = rt.load_renderer(text)
        rt.set_lights(f.lights)
        d_raw = torch.from_numpy(raw).cuda()
        rt.set_render_target("DepthBuffer", d_raw)
        surface = torch.from_numpy(f.surface).cuda()
        chain = torch.full((host.mip_chain_texels(W, H, levels) * 4,), -3.0, dtype=torch.float32, device="cuda")
        radiance = chain[:W * H * 4].view(H, W, 4)                   # level 0 of Main is the buffer RenderScene writes
        rt.set_surface(surface, radiance)
        rt.set_color_target_chain("Main", chain, W, H, levels)
        rt.set_time(1.0 / 60.0, 0.0)
        assert rt.process_frame() == 0
        rt.wait_idle()
        torch.cuda.synchronize()
        return loaded, chain.cpu().numpy()
    finally:
        rt.close()


def test_bloom_behind_the_render_scene_pass():
    """RenderScene in front: one run without the opt-in reads the radiance (the entry is skipped, level 0 of Main is what the shade wrote); the run
    with the opt-in must leave the restatement's chain of that radiance in Main.  The first run is used as long as the shade is bit-reproducible,
    which a second run without the opt-in establishes; were it not, this step would be skipped and say so."""
    f = synth.make_frame("tiny")
    W, H, levels = f.cam.width, f.cam.height, 5
    params = dict(threshold=0.3, knee=0.2, bloom_intensity=1.3, dirt_intensity=5.0)   # the tiny frame's lights are not saturated: a lower threshold
    text = HEAD + RENDER_SCENE + BLOOM_AND_EYE_ADAPTATION % params
    raw = synth.make_raw_depth(f.depth, f.cam.frame.cameraZNearZFar[0])
    dirt = make_dirt()
    loaded, plain = run_tiny_frame(text, f, raw, levels, False, dirt)
    assert loaded[:2] == (4, 1)
    _, again = run_tiny_frame(text, f, raw, levels, False, dirt)
    n0 = W * H * 4
    if not np.array_equal(plain[:n0].view(np.uint32), again[:n0].view(np.uint32)):
        pytest.skip("the shade is not bit-reproducible from run to run here: no radiance to restate the bloom of")
    assert (plain[n0:] == F(-3.0)).all(), "without the node nobody writes the lower levels"
    radiance = plain[:n0].reshape(H, W, 4)
    assert np.isfinite(radiance).all() and radiance[..., :3].max() > 0
    want = ref.bloom_chain(radiance, levels, dirt=dirt, **params)
    assert (want[1][..., :3] != 0).any(axis=-1).mean() > 0.05, "the frame must bloom for this to show anything"
    loaded, bloomed = run_tiny_frame(text, f, raw, levels, True, dirt)
    assert loaded[:2] == (5, 0)
    for l, (got, wnt) in enumerate(zip(ref.split(bloomed, W, H, levels), want)):
        ok, msg = ref.same_bits(got, wnt)
        assert ok, f"level {l} of Main: {msg}"
