"""GPU suite of the EyeAdaptation kernels through the C-ABI (sailor_hip_luminance_histogram, sailor_hip_average_luminance, sailor_hip_tonemap,
sailor_hip_eye_adaptation) against the fp32 restatement of tests/eye_adaptation_ref.py, BIT FOR BIT: the 256 counts, the adapted-luminance
word and the LDR image (non-finite values compared by class, as tests/test_shade_gpu.py compares them)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import eye_adaptation_ref as ref
from eye_adaptation_ref import Ref32
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import EyeAdaptation, ForwardPlus, HipContext, upload_lights, upload_shadow_maps

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def shaded_radiance(ctx, name):
    """the radiance of a synthetic frame as the shade kernels produce it (H x W x 4 device tensor)"""
    f = synth.make_frame(name)
    fp = ForwardPlus(ctx, f.cam.width, f.cam.height, len(f.lights))
    d = torch.from_numpy(f.depth).to(ctx.device)
    s = torch.from_numpy(f.surface).to(ctx.device)
    l = upload_lights(f.lights, ctx.device)
    fp.cull(f.cam.frame, l, len(f.lights), d)
    desc, keep = upload_shadow_maps(f.shadows, ctx.device) if f.shadows is not None else (None, None)
    out = fp.shade(f.cam.frame, s, l, len(f.lights), desc).clone()
    ctx.synchronize()
    return out


def constants_tuple(c):
    return f32(c.minLog2Luminance), f32(c.invLog2LuminanceRange), f32(c.log2LuminanceRange), f32(c.numPixels), f32(c.timeCoeff)


def random_image(h, w, seed):
    rng = np.random.default_rng(seed)
    img = np.exp2(rng.uniform(-12.0, 7.0, (h, w, 4))).astype(f32)
    img[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(f32)
    return img


def assert_step_matches(ctx, image, ops_sets=ref.OPERATOR_SETS, delta_time=1.0 / 60.0, initial=0.5):
    """one frame of the node per operator set: counts, luminance word, LDR image against the restatement (the host's constants feed both)"""
    img_np = image.cpu().numpy() if isinstance(image, torch.Tensor) else image
    img = image if isinstance(image, torch.Tensor) else torch.from_numpy(image).to(ctx.device)
    h, w = img_np.shape[:2]
    for ops in ops_sets:
        names = " ".join(n for n, b in _lib.TONEMAP_DEFINES.items() if ops & b)
        ea = EyeAdaptation(ctx, w, h, defines=names, initial_luminance=initial)
        k = ea.constants(delta_time)
        # the three entry points one by one, so that the counts can be read before the average clears them
        ea.histogram(img, k)
        ctx.synchronize()
        counts = ea.views()[0].cpu().numpy().view(np.uint32).copy()
        ea.average(k)
        ldr = ea.tonemap(img)
        ctx.synchronize()
        got_counts_after, got_lum = ea.views()[0].cpu().numpy(), ea.views()[1].cpu().numpy()
        want_counts, want_lum, want_ldr = ref.step(Ref32, img_np, initial, delta_time, ops, constants=constants_tuple(k))
        np.testing.assert_array_equal(counts, want_counts)
        assert not got_counts_after.any(), "the average pass zeroes the histogram for the next frame"
        assert got_lum.view(np.uint32)[0] == f32(want_lum).view(np.uint32), (ops, got_lum, want_lum)
        ok = ref.same_bits_or_class(ldr.cpu().numpy(), want_ldr)
        assert ok.all(), f"ops {ops}: {int((~ok).sum())} of {ok.size} LDR values differ from the restatement"
        # the node's one-call form leaves the same words
        ea2 = EyeAdaptation(ctx, w, h, defines=names, initial_luminance=initial)
        ldr2 = ea2.run(img, delta_time)
        ctx.synchronize()
        assert torch.equal(ldr2.view(torch.int32), ldr.view(torch.int32)) and torch.equal(ea2.state, ea.state)


@pytest.mark.parametrize("name", ["tiny", "tiny_csm"])
def test_shaded_tiny_frames_all_operator_sets(ctx, name):
    assert_step_matches(ctx, shaded_radiance(ctx, name))


def test_stored_fixture(ctx):
    g = np.load(ROOT / "tests" / "golden" / "tiny_tonemap.npz")
    rad = torch.from_numpy(g["radiance"]).to(ctx.device)
    h, w = g["radiance"].shape[:2]
    for ops in ref.OPERATOR_SETS:
        ea = EyeAdaptation(ctx, w, h, defines=" ".join(n for n, b in _lib.TONEMAP_DEFINES.items() if ops & b), initial_luminance=float(g["initial_luminance"]))
        k = ea.constants(float(g["delta_time"]))
        k.timeCoeff = float(g["constants"][4])  # the stored constants (the host's exp2f may sit an ulp from the generator's)
        ea.histogram(rad, k)
        ctx.synchronize()
        np.testing.assert_array_equal(ea.views()[0].cpu().numpy().view(np.uint32), g["counts"])
        ea.average(k)
        ldr = ea.tonemap(rad).cpu().numpy()
        assert ea.views()[1].cpu().numpy().view(np.uint32)[0] == g["luminance"].view(np.uint32)
        assert ref.same_bits_or_class(ldr, g[f"ldr_{ops}"]).all()


@pytest.mark.parametrize("size", [(100, 52), (333, 77), (16, 16), (15, 40), (1031, 19)])
def test_ragged_sizes(ctx, size):
    """the right / bottom remainder of a size that is no multiple of 16 is not counted; numPixels stays width x height"""
    w, h = size
    img = random_image(h, w, 1000 + w)
    img[h // 16 * 16:, :, :3] = 1000.0
    img[:, w // 16 * 16:, :3] = 1000.0
    assert_step_matches(ctx, img, ops_sets=(ref.UNCHARTED2 | ref.LUMINANCE, ref.ACES))


def test_whole_4k_frame_of_c3_radiance(ctx):
    rad = shaded_radiance(ctx, "C3")
    assert tuple(rad.shape) == (2160, 3840, 4)
    assert_step_matches(ctx, rad, ops_sets=(ref.UNCHARTED2 | ref.LUMINANCE, ref.ACES))


def hostile_image():
    """NaN, +-inf, negatives, exact black, values beyond both ends of the range, and one-bin constant rows"""
    img = random_image(64, 256, 5)
    img[8:40, :, :3] = 0.3           # one-bin constant block (whole waves on one bin)
    img[40:44, :, :3] = 0.0          # exact black: NaN under LUMINANCE
    rng = np.random.default_rng(6)
    specials = np.array([np.nan, np.inf, -np.inf, -3.0, 0.0, -0.0, 3.0e38, 1.0e-30, 1.0e-45, 65504.0, 0.005, 0.0049999], f32)
    img[44:52, :, :3] = specials[rng.integers(0, len(specials), (8, 256, 3))]
    img[52, :12, :3] = specials[:, None]
    img[53, :, 3] = np.nan           # alpha passes through
    return img


def test_hostile_image(ctx):
    img = hostile_image()
    assert_step_matches(ctx, img)
    counts = Ref32.histogram(img)
    assert counts.sum() == 64 * 256 and counts[0] > 4 * 256 and counts[255] > 0


@pytest.mark.parametrize("size", [(128, 96), (1280, 720), (100, 52), (3840, 2160)])
def test_bands_accumulate_to_the_whole_frame(ctx, size):
    """the histograms of the eight bands of sailor_hip_band_for_rank accumulated into ONE state are the whole frame's counts; banded tone-map rows
    are the whole frame's rows"""
    w, h = size
    img_np = random_image(h, w, 77 + w)
    img = torch.from_numpy(img_np).to(ctx.device)
    whole = EyeAdaptation(ctx, w, h)
    k = whole.constants(0.02)
    whole.histogram(img, k)
    ctx.synchronize()
    whole_counts = whole.views()[0].cpu().numpy().copy()
    np.testing.assert_array_equal(whole_counts.view(np.uint32), Ref32.histogram(img_np))
    whole.average(k)
    whole_ldr = whole.tonemap(img)
    banded = EyeAdaptation(ctx, w, h)
    bands = [host.band_for_rank(w, h, r, 8) for r in range(8)]
    assert sum(b.fbRowCount for b in bands) == h
    parts = [img[b.fbRowBegin:b.fbRowBegin + b.fbRowCount].contiguous() for b in bands]
    for b, p in zip(bands, parts):
        banded.histogram(p, k, band=b)
    ctx.synchronize()
    np.testing.assert_array_equal(banded.views()[0].cpu().numpy(), whole_counts)
    banded.average(k)
    for b, p in zip(bands, parts):
        rows = banded.tonemap(p, band=b)
        assert torch.equal(rows.view(torch.int32), whole_ldr[b.fbRowBegin:b.fbRowBegin + b.fbRowCount].view(torch.int32))
    ctx.synchronize()
    assert torch.equal(banded.state, whole.state)


def ten_frames(seed=11):
    """ten images and frame times that change from frame to frame (a scene that brightens, darkens and cuts to black)"""
    base = random_image(96, 160, seed)
    gains = [1.0, 4.0, 16.0, 0.25, 0.01, 0.0, 1.0, 300.0, 1.0e-3, 2.0]
    dts = [1 / 60, 1 / 30, 0.1, 1 / 144, 0.5, 1 / 60, 2.0, 0.004, 1 / 60, 0.0]
    frames = []
    for g in gains:
        img = base.copy()
        img[..., :3] *= f32(g)
        frames.append(img)
    return frames, dts


def test_ten_frames_eager_and_captured(ctx):
    """ten frames with a changing image and deltaTime: eager == ten steps of the restatement; the same thirty launches captured ONCE into a
    hipGraph (a linear chain) and replayed leave the same words"""
    frames, dts = ten_frames()
    h, w = frames[0].shape[:2]
    imgs = [torch.from_numpy(f).to(ctx.device) for f in frames]
    ea = EyeAdaptation(ctx, w, h)
    lum, eager_ldr, eager_lum = 0.5, [], []
    for img_np, img, dt in zip(frames, imgs, dts):
        k = ea.constants(dt)
        out = ea.run(img, dt)
        ctx.synchronize()
        got = ea.views()[1].cpu().numpy().view(np.uint32)[0]
        _, lum, want = ref.step(Ref32, img_np, lum, dt, ref.UNCHARTED2 | ref.LUMINANCE, constants=constants_tuple(k))
        assert got == f32(lum).view(np.uint32), (dt, got, lum)
        assert ref.same_bits_or_class(out.cpu().numpy(), want).all()
        eager_ldr.append(out)
        eager_lum.append(got)
    assert len(set(eager_lum)) > 5, "the luminance moves from frame to frame"

    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        ea2 = EyeAdaptation(c2, w, h)
        outs = [torch.zeros_like(i) for i in imgs]
        lums = torch.zeros(10, dtype=torch.int32, device=ctx.device)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            ea2.reset(0.5)
            for i, (img, dt) in enumerate(zip(imgs, dts)):
                ea2.run(img, dt, out=outs[i])
                lums[i:i + 1].copy_(ea2.views()[1].view(torch.int32))
        for _ in range(2):  # the graph starts from its own reset: a second replay leaves the same words
            graph.replay()
            torch.cuda.synchronize()
            assert [int(v) for v in lums.cpu().numpy().view(np.uint32)] == [int(v) for v in eager_lum]
            for a, b in zip(outs, eager_ldr):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        c2.close()


def test_the_weighted_sum_wraps_at_8k_on_the_device(ctx):
    """counts uploaded directly: 7680 x 4320 pixels in bin 255 give a uint32 sum of 4 165 320 704, not 8 460 288 000"""
    ea = EyeAdaptation(ctx, 7680, 4320)
    k = ea.constants(1.0)
    for counts in (np.eye(1, 256, 255, dtype=np.uint32)[0] * np.uint32(7680 * 4320), np.full(256, 7680 * 4320 // 256, np.uint32)):
        ea.reset(0.5)
        ea.views()[0].copy_(torch.from_numpy(counts.view(np.int32)).to(ctx.device))
        ea.average(k)
        ctx.synchronize()
        want = Ref32.average(counts, 0.5, *[constants_tuple(k)[i] for i in (0, 2, 3, 4)])
        assert ea.views()[1].cpu().numpy().view(np.uint32)[0] == f32(want).view(np.uint32)
        assert not ea.views()[0].cpu().numpy().any()
    assert int(ref.weighted_sum_u32(np.eye(1, 256, 255, dtype=np.uint32)[0] * np.uint32(7680 * 4320))) == 4165320704


def test_argument_checks_refuse_without_launching(ctx):
    lib = ctx._lib
    w, h = 64, 32
    img = torch.from_numpy(random_image(h, w, 3)).to(ctx.device)
    out = torch.zeros_like(img)
    ea = EyeAdaptation(ctx, w, h)
    k = ea.constants(0.1)
    band = host.band_whole_frame(w, h)
    wp = (C.c_float * 4)(1.4, 1.5, 1.4, 0.0)
    st, col, dst = ea.state.data_ptr(), img.data_ptr(), out.data_ptr()
    ctx.synchronize()
    before_state = ea.state.clone()
    bad_band = _lib.Band(0, 1, 0, 16)  # not what the band helpers produce for this size
    other = host.band_whole_frame(w, h + 16)

    def calls():
        kb, bb = C.byref(k), C.byref(band)
        H, A, T, E = lib.sailor_hip_luminance_histogram, lib.sailor_hip_average_luminance, lib.sailor_hip_tonemap, lib.sailor_hip_eye_adaptation
        yield H(ctx.handle, None, w, h, bb, kb, st)             # null pointers
        yield H(ctx.handle, col, w, h, None, kb, st)
        yield H(ctx.handle, col, w, h, bb, None, st)
        yield H(ctx.handle, col, w, h, bb, kb, None)
        yield H(ctx.handle, col + 4, w, h, bb, kb, st)          # misaligned pointers
        yield H(ctx.handle, col, w, h, bb, kb, st + 4)
        yield H(ctx.handle, col, 0, h, bb, kb, st)              # sizes
        yield H(ctx.handle, col, w, h, C.byref(bad_band), kb, st)
        yield H(ctx.handle, col, w, h, C.byref(other), kb, st)  # a band of another frame size
        yield A(ctx.handle, None, st)
        yield A(ctx.handle, kb, None)
        yield A(ctx.handle, kb, st + 8)
        yield T(ctx.handle, None, dst, w, h, bb, 6, wp, 1.0, st)
        yield T(ctx.handle, col, None, w, h, bb, 6, wp, 1.0, st)
        yield T(ctx.handle, col, dst, w, h, bb, 6, None, 1.0, st)
        yield T(ctx.handle, col, dst, w, h, bb, 6, wp, 1.0, None)
        yield T(ctx.handle, col, dst + 8, w, h, bb, 6, wp, 1.0, st)
        yield T(ctx.handle, col, col, w, h, bb, 6, wp, 1.0, st)  # source and target are two images
        yield T(ctx.handle, col, dst, w, h, C.byref(other), 6, wp, 1.0, st)  # differing source and target sizes
        yield T(ctx.handle, col, dst, w, h, bb, 8, wp, 1.0, st)  # an unknown operator flag
        yield T(ctx.handle, col, dst, w, h, bb, 0x16, wp, 1.0, st)
        yield E(ctx.handle, col, dst, w, h, kb, 8, wp, 1.0, st)
        yield E(ctx.handle, col, dst + 4, w, h, kb, 6, wp, 1.0, st)
        yield E(ctx.handle, col, dst, w, -1, kb, 6, wp, 1.0, st)
        yield E(ctx.handle, None, dst, w, h, kb, 6, wp, 1.0, st)
        yield lib.sailor_hip_eye_adaptation_reset(ctx.handle, None, 0.5)
        yield lib.sailor_hip_eye_adaptation_reset(ctx.handle, st + 4, 0.5)

    launched_before, _ = ctx.launch_log(0)
    statuses = list(calls())
    assert statuses == [-1] * len(statuses), statuses
    assert ctx.launch_log(0)[0] == launched_before, "a refused call launches nothing"
    ctx.synchronize()
    assert torch.equal(ea.state, before_state) and not out.any()
    # and the kernels are named in the launch log
    assert ctx.launches_of(lambda: ea.run(img, 0.1, out=out)) == ["k_luminance_histogram", "k_average_luminance", "k_tonemap"]
