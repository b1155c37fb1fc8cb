"""The post effects through the C++ host mirror (GPU): a `.renderer` text of its own -- Blit Main -> Quarter1 (Linear), Blur HORIZONTAL and VERTICAL
between the quarter targets, Blur RADIAL back to full size, ChromaticAberation into BackBuffer -- loaded through Runtime.load_renderer WITHOUT any
opt-in.  BlitNode and PostProcessNode record the reference's call sequence; the HIP backend routes the five commands to sailor_hip_blit_linear,
sailor_hip_blur and sailor_hip_chromatic_aberration.  Every target must equal the chained fp32 restatement (tests/effects_ref.py) bit for bit."""
import numpy as np
import pytest
import torch

import effects_cases as ec
import effects_ref as ref
from effects_ref import Ref32
from sailor_amd.forward_plus import evsm_blur_pass
from sailor_amd.runtime_binding import Runtime
from tail_cases import camera
from test_runtime_gpu import read_u32

pytestmark = pytest.mark.gpu
f32 = np.float32
W, H, QW, QH = 131, 77, 64, 48
FIVE = ["k_blit_linear", "k_blur_gauss", "k_blur_gauss", "k_blur_radial", "k_chromatic_aberration"]

TARGETS = """---
renderTargets:
- name: Quarter1
  format: R16G16B16A16_SFLOAT
  width: %d
  height: %d

- name: Quarter2
  format: R16G16B16A16_SFLOAT
  width: %d
  height: %d

- name: Blurred
  format: R16G16B16A16_SFLOAT
  width: ViewportWidth
  height: ViewportHeight

frame:
""" % (QW, QH, QW, QH)
BLIT = """- name: Blit
  renderTargets:
  - src: Main
  - dst: Quarter1

"""
BLUR = """- name: PostProcess
  string:
  - shader: Shaders/Blur.shader
  - defines: %s
  vec4:
  - data.blurRadius: [%s, 2, 0, 0]
  renderTargets:
  - colorSampler: %s
  - color: %s

"""
RADIAL = """- name: PostProcess
  string:
  - shader: Shaders/Blur.shader
  - defines: RADIAL
  vec4:
  - data.blurRadius: [20, 0, 0, 0]
  - data.blurSampleCount: [10, 0, 0, 0]
  - data.blurCenter: [0.5, 0.5, 0, 0]
  renderTargets:
  - colorSampler: Quarter1
  - color: Blurred

"""
ABERRATION = """- name: PostProcess
  string:
  - shader: Shaders/ChromaticAberation.shader
  - defines: ~
  vec4:
  - data.offset: [0.00225, 0.00345, 0.00455, 0.0]
  renderTargets:
  - color: BackBuffer
  - depthStencil: DepthBuffer
  - colorSampler: Blurred
"""
CHAIN = TARGETS + BLIT + BLUR % ("HORIZONTAL", 4, "Quarter1", "Quarter2") + BLUR % ("VERTICAL", 4, "Quarter2", "Quarter1") + RADIAL + ABERRATION


class Frame:
    """a runtime with Main (the caller's RGBA32F plane, alpha neither 0 nor 1) and BackBuffer (-3 everywhere) bound; no scene, no lights, no opt-in"""

    def __init__(self, text):
        self.rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        self.rt.set_camera(camera(W, H))
        self.loaded = self.rt.load_renderer(text)
        self.main_host = ec.plane((W, H), 30)
        self.main = torch.from_numpy(self.main_host).cuda()
        self.back = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
        self.rt.set_color_target("Main", self.main)
        self.rt.set_color_target("BackBuffer", self.back)

    def process(self):
        st = self.rt.process_frame()
        self.rt.wait_idle()
        torch.cuda.synchronize()
        return st

    def target(self, name, w, h):
        p, tw, th, _ = self.rt.render_target(name)
        assert p and (tw, th) == (w, h), (name, tw, th)
        return read_u32(p, w * h * 16).view(f32).reshape(h, w, 4)

    def close(self):
        self.rt.close()


def same_words(got, want, what):
    ok = np.ascontiguousarray(got, f32).view(np.uint32) == np.ascontiguousarray(want, f32).view(np.uint32)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} words differ from the restatement, first at {tuple(np.argwhere(~ok)[0])}"


def test_the_chain_into_backbuffer():
    """fails without the feature: the parent refuses the scaled Linear blit and the blurs' parameters, and records nothing for the aberration"""
    fr = Frame(CHAIN)
    try:
        assert fr.loaded[:2] == (5, 0)
        for k in range(2):   # a second frame records the same five launches and, Main being the caller's, the same images
            before, _ = fr.rt.launch_log(0)
            assert fr.process() == 0
            after, names = fr.rt.launch_log(16)
            assert after - before == 5 and names[-5:] == FIVE, names
        q1 = Ref32.blit_linear(fr.main_host, QW, QH)
        q2 = Ref32.blur(q1, dict(blurRadius=4.0), ref.HORIZONTAL, QW, QH)
        q1 = Ref32.blur(q2, dict(blurRadius=4.0), ref.VERTICAL, QW, QH)
        blurred = Ref32.blur(q1, ref.RADIAL_SHIPPED, ref.RADIAL, W, H)
        back = Ref32.chromatic_aberration(blurred, ref.ABERRATION_SHIPPED, W, H)
        same_words(fr.target("Quarter2", QW, QH), q2, "Quarter2: Blit, Blur HORIZONTAL")
        same_words(fr.target("Quarter1", QW, QH), q1, "Quarter1: ... Blur VERTICAL")
        same_words(fr.target("Blurred", W, H), blurred, "Blurred: ... Blur RADIAL")
        same_words(fr.back.cpu().numpy(), back, "BackBuffer: ... ChromaticAberation")
        assert (q1[..., 3] == 0).all() and (blurred[..., 3] == 0).all() and (back[..., 3] == 1).all() and back[..., :3].max() > 1.0
        assert np.array_equal(fr.main.cpu().numpy(), fr.main_host), "Main is only read"
    finally:
        fr.close()


def test_evsm_with_a_direction_still_records_the_evsm_blur(ctx):
    """k_evsm_blur is launched outside the launch log (sailor_amd/csrc/shadow_blur.hip), so it is known by what it leaves: Quarter2 holds the bits of
    sailor_hip_evsm_blur_pass over the blit's output -- all four channels, alpha included -- and no Gauss kernel was recorded"""
    fr = Frame(TARGETS + BLIT + BLUR % ("EVSM HORIZONTAL", 2, "Quarter1", "Quarter2"))
    try:
        assert fr.process() == 0
        _, names = fr.rt.launch_log(16)
        assert names[-1] == "k_blit_linear" and "k_blur_gauss" not in names, names
        q1 = Ref32.blit_linear(fr.main_host, QW, QH)
        want = evsm_blur_pass(ctx, torch.from_numpy(q1).to(ctx.device), 2, 2, False)   # ivec2(data.blurRadius.xy) = (2, 2)
        ctx.synchronize()
        want = want.cpu().numpy()
        same_words(fr.target("Quarter2", QW, QH), want, "Quarter2: Blit, Blur EVSM HORIZONTAL")
        assert (want[..., 3] != 0).all(), "the EVSM blur writes alpha"
    finally:
        fr.close()


def test_radial_wins_over_evsm():
    fr = Frame(TARGETS + BLIT + RADIAL.replace("defines: RADIAL", "defines: EVSM RADIAL"))
    try:
        assert fr.process() == 0
        _, names = fr.rt.launch_log(16)
        assert names[-2:] == ["k_blit_linear", "k_blur_radial"], names
    finally:
        fr.close()


def test_enable_shader_still_raises_for_the_new_shaders():
    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        for path in ("Shaders/ChromaticAberation.shader", "Shaders/Blur.shader"):
            with pytest.raises(ValueError):
                rt.enable_shader(path)
    finally:
        rt.close()


def test_an_unresolved_color_sampler_fails_the_frame_and_writes_nothing():
    fr = Frame(TARGETS + BLUR % ("HORIZONTAL", 4, "NoSuchTarget", "BackBuffer"))
    try:
        assert fr.process() == -1   # SAILOR_HIP_ERR_INVALID_ARGUMENT
        count, names = fr.rt.launch_log(16)
        assert "k_blur_gauss" not in names, names
        assert (fr.back == -3.0).all()
    finally:
        fr.close()
