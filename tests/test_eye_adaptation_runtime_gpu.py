"""The EyeAdaptation node through the C++ host mirror (GPU): a `.renderer` description of its own with LinearizeDepth -> LightCulling ->
RenderScene -> EyeAdaptation and the shipped parameters (tests/golden/DefaultRenderer.renderer:307-319), loaded through Runtime.load_renderer.
The node records the reference's call sequence against the mirrored RHI (two Dispatches, one full-screen draw); the HIP backend routes them to
sailor_hip_luminance_histogram / sailor_hip_average_luminance / sailor_hip_tonemap.  The LDR target and the adapted luminance must equal the fp32
restatement (tests/eye_adaptation_ref.py) applied to the radiance the same graph produced, bit for bit."""
import numpy as np
import pytest
import torch

import eye_adaptation_ref as ref
from eye_adaptation_ref import Ref32
from sailor_amd import host, synth
from sailor_amd.runtime_binding import Runtime, parse_renderer
from test_runtime_gpu import read_u32

pytestmark = pytest.mark.gpu
f32 = np.float32

EYE_ADAPTATION_RENDERER = """---
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
- name: LinearizeDepth
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

- name: EyeAdaptation
  string:
  - toneMappingShader: Shaders/Tonemapping.shader
  - toneMappingDefines: %s
  vec4:
  - data.exposure: [%s, 0, 0, 0]
  - data.whitePoint: [1.4, 1.5, 1.4, 0]
  renderTargets:
  - color: Secondary
  - hdrColor: Main
  - colorSampler: Main
  - depthStencil: DepthBuffer
"""


def constants_tuple(c):
    return f32(c.minLog2Luminance), f32(c.invLog2LuminanceRange), f32(c.log2LuminanceRange), f32(c.numPixels), f32(c.timeCoeff)


@pytest.mark.parametrize("defines,exposure", [("UNCHARTED2 LUMINANCE", 1.0), ("ACES", 1.0), ("UNCHARTED2", 0.75)])
def test_eye_adaptation_node_behind_the_render_scene_pass(defines, exposure):
    text = EYE_ADAPTATION_RENDERER % (defines, exposure)
    n, summary = parse_renderer(text, 128, 96)
    assert n == 4 and "EyeAdaptation[]" in summary and "string toneMappingDefines=" + defines in summary
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    zn = f.cam.frame.cameraZNearZFar[0]
    raw = synth.make_raw_depth(f.depth, zn)
    ops = sum({"ACES": ref.ACES, "UNCHARTED2": ref.UNCHARTED2, "LUMINANCE": ref.LUMINANCE}[d] for d in defines.split())
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(f.cam)
        created, skipped, targets = rt.load_renderer(text)
        assert (created, skipped, targets) == (4, 0, 2)   # EyeAdaptation has a node class: created, not skipped
        rt.set_lights(f.lights)
        d_raw = torch.from_numpy(raw).cuda()
        rt.set_render_target("DepthBuffer", d_raw)
        surface = torch.from_numpy(f.surface).cuda()
        radiance = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rt.set_surface(surface, radiance)
        rt.set_color_target("Main", radiance)             # the HDR target the RenderScene pass writes
        ldr_ptr, w, h, levels = rt.render_target("Secondary")
        assert ldr_ptr and (w, h, levels) == (W, H, 1)
        dts = (1.0 / 60.0, 0.25)
        want_lum, want_ldr = f32(0.5), None
        for i, dt in enumerate(dts):
            rt.set_time(dt, 0.1 * i)
            assert rt.process_frame() == 0
            rt.wait_idle()
            torch.cuda.synchronize()
            rad = radiance.cpu().numpy()
            assert np.isfinite(rad).all() and rad[..., :3].max() > 0
            k = constants_tuple(host.eye_adaptation_constants(W, H, dt))
            counts, want_lum, want_ldr = ref.step(Ref32, rad, want_lum, dt, ops, exposure=exposure, constants=k)
            hist_ptr, lum_ptr = rt.eye_adaptation_state()
            assert read_u32(lum_ptr, 4)[0] == f32(want_lum).view(np.uint32), (i, want_lum)
            assert not read_u32(hist_ptr, 1024).any(), "the average pass leaves the histogram zeroed for the next frame"
            assert counts.sum() == W * H
            got = read_u32(ldr_ptr, W * H * 16).view(f32).reshape(H, W, 4)
            assert ref.same_bits_or_class(got, want_ldr).all(), f"frame {i}: the LDR target differs from the restatement"
        assert f32(want_lum) != f32(0.5)
    finally:
        rt.close()


def test_a_tone_mapping_source_of_another_size_is_refused():
    """the draw is a texel fetch of a same-size source: a `colorSampler` of another size than `color` is refused with the invalid-argument status"""
    text = EYE_ADAPTATION_RENDERER % ("UNCHARTED2 LUMINANCE", 1.0)
    f = synth.make_frame("tiny")
    W, H = f.cam.width, f.cam.height
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(f.cam)
        rt.load_renderer(text)
        rt.set_lights(f.lights)
        rt.set_render_target("DepthBuffer", torch.from_numpy(synth.make_raw_depth(f.depth, 1.0)).cuda())
        surface = torch.from_numpy(f.surface).cuda()
        radiance = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rt.set_surface(surface, radiance)
        rt.set_color_target("Main", torch.zeros((H // 2, W // 2, 4), dtype=torch.float32, device="cuda"))
        assert rt.process_frame() == -1
        rt.wait_idle()
    finally:
        rt.close()
