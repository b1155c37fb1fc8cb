"""GPU suite of the HBAO kernels through the C-ABI (sailor_hip_blit_nearest, sailor_hip_hbao, sailor_hip_hbao_blur_pass, sailor_hip_hbao_chain)
against the fp32 restatement of tests/hbao_ref.py, BIT FOR BIT: the planes are compared as uint32 words (the store maps NaN to 0, so no plane
holds a non-finite value)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import hbao_ref as ref
from hbao_cases import OTHER, OTHER_BLUR, hostile_depth, is_lively, noise_texels, raw_depth
from hbao_ref import Ref32
from oracle import oracle
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import ForwardPlus, Hbao, HipContext, upload_ibl, upload_lights

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.cpu().numpy()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    bad = bits(g) != bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ from the restatement, first at {tuple(np.argwhere(bad)[0])}"


def make_hbao(ctx, w, h, params=None, blur=None, extents=None):
    noise = torch.from_numpy(noise_texels()).to(ctx.device)
    return Hbao(ctx, w, h, noise, params=host.hbao_params(**(params or {})), blur_params=host.hbao_blur_params(**(blur or {})), extents=extents)


def check_all(ctx, frame, raw, w, h, extents, params=None, blur=None, lively=True):
    """each entry point on the restatement's inputs, then the chain: all four planes bit for bit"""
    P, B = dict(ref.SHIPPED, **(params or {})), dict(ref.SHIPPED_BLUR, **(blur or {}))
    want = Ref32.chain(frame, raw, noise_texels(), P, B, *extents)
    if lively:
        assert is_lively(want[1]), "parity on a blank plane shows nothing"
    hb = make_hbao(ctx, w, h, params, blur, extents)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, f32)).to(ctx.device)
    d = dev(raw)
    same_bits(hb.blit(d, torch.zeros_like(hb.half_depth)), want[0], "blit")
    same_bits(hb.hbao(frame, dev(want[0]), torch.zeros_like(hb.ao)), want[1], "hbao")
    same_bits(hb.blur_pass(dev(want[1]), d, torch.zeros_like(hb.temp), True), want[2], "vertical blur")
    same_bits(hb.blur_pass(dev(want[2]), d, torch.zeros_like(hb.g_ao), False), want[3], "horizontal blur")
    out = hb.run(frame, d)
    ctx.synchronize()
    assert out.data_ptr() == hb.g_ao.data_ptr()
    for got, w_, name in zip((hb.half_depth, hb.ao, hb.temp, hb.g_ao), want, ("HalfDepth", "AO", "TemporaryR8", "g_AO")):
        same_bits(got, w_, f"chain {name}")
    return want


def test_tiny_frame_shipped_extents_and_golden(ctx):
    cam, raw = raw_depth(128, 96)
    want = check_all(ctx, cam.frame, raw, 128, 96, ref.shipped_extents(128, 96))
    gold = np.load(ROOT / "tests" / "golden" / "tiny_hbao.npz")
    hb = make_hbao(ctx, 128, 96, extents=ref.shipped_extents(128, 96))
    hb.run(cam.frame, torch.from_numpy(raw).to(ctx.device))
    ctx.synchronize()
    np.testing.assert_array_equal(bits(hb.half_depth.cpu().numpy()), gold["half_depth_bits"])
    for name, plane in (("ao", hb.ao), ("temp", hb.temp), ("g_ao", hb.g_ao)):
        np.testing.assert_array_equal(ref.codes(plane.cpu().numpy()), gold[name])
        np.testing.assert_array_equal(bits(plane.cpu().numpy()), bits((gold[name].astype(f32) / f32(255.0))))
    assert np.array_equal(ref.codes(want[3]), gold["g_ao"])


def test_ragged_frame(ctx):
    cam, raw = raw_depth(131, 77)
    check_all(ctx, cam.frame, raw, 131, 77, ref.shipped_extents(131, 77))


def test_extents_independent_of_one_another(ctx):
    """AO extent different from the depth extent, frame-sized g_AO, and the other parameter set"""
    cam, raw = raw_depth(128, 96)
    check_all(ctx, cam.frame, raw, 128, 96, ((64, 48), (50, 70), (128, 96), (128, 96)), OTHER, OTHER_BLUR)
    check_all(ctx, cam.frame, raw, 128, 96, ((61, 37), (97, 33), (45, 101), (128, 96)))


def test_shipped_extents_for_a_256x144_viewport(ctx):
    cam, raw = raw_depth(256, 144)
    ext = ref.shipped_extents(256, 144)
    assert ext == ((128, 128), (128, 128), (256, 256), (256, 256)) and ext == host.hbao_shipped_extents(256, 144)
    check_all(ctx, cam.frame, raw, 256, 144, ext)
    check_all(ctx, cam.frame, raw, 256, 144, ext, OTHER, OTHER_BLUR)


def test_depth_with_sky_blocks(ctx):
    cam, raw = raw_depth(256, 144, sky_fraction=0.2)
    assert (raw == 0).mean() > 0.1
    want = check_all(ctx, cam.frame, raw, 256, 144, ref.shipped_extents(256, 144))
    assert (want[1] == 1.0).mean() > 0.05, "the sky check stores 1"


def test_hostile_depth(ctx):
    """0, 1, denormals, +inf and NaN texels: compared by bits; no plane holds a non-finite value"""
    cam, raw = hostile_depth(131, 77)
    want = check_all(ctx, cam.frame, raw, 131, 77, ref.shipped_extents(131, 77), lively=False)
    assert all(np.isfinite(p).all() for p in want[1:])


def test_full_hd_depth(ctx):
    """the C3 depth at 1080p with the shipped extents (the restatement needs minutes for the 4K planes, so the large case is 1080p)"""
    cam, raw = raw_depth(1920, 1080)
    P, B = ref.SHIPPED, ref.SHIPPED_BLUR
    ext = ref.shipped_extents(1920, 1080)
    want = Ref32.chain(cam.frame, raw, noise_texels(), P, B, *ext)
    assert is_lively(want[1])
    hb = make_hbao(ctx, 1920, 1080, extents=ext)
    hb.run(cam.frame, torch.from_numpy(raw).to(ctx.device))
    ctx.synchronize()
    for got, w_, name in zip((hb.half_depth, hb.ao, hb.temp, hb.g_ao), want, ("HalfDepth", "AO", "TemporaryR8", "g_AO")):
        same_bits(got, w_, name)


def test_ten_frames_eager_and_replayed_from_one_graph(ctx):
    w, h = 128, 96
    cams, raws = zip(*[raw_depth(w, h, seed=100 + i, sky_fraction=0.1 * (i % 3)) for i in range(10)])
    depths = [torch.from_numpy(r).to(ctx.device) for r in raws]
    hb = make_hbao(ctx, w, h)
    eager = []
    for cam, d in zip(cams, depths):
        eager.append(hb.run(cam.frame, d).clone())
    ctx.synchronize()
    assert len({e.cpu().numpy().tobytes() for e in eager}) == 10
    same_bits(eager[3], Ref32.chain(cams[3].frame, raws[3], noise_texels(), ref.SHIPPED, ref.SHIPPED_BLUR, *hb.extents)[3], "frame 3")

    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        hb2 = make_hbao(c2, w, h)
        outs = [torch.zeros_like(e) for e in eager]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for cam, d, o in zip(cams, depths, outs):
                o.copy_(hb2.run(cam.frame, d))
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(outs, eager):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    finally:
        c2.close()


def test_chain_output_feeds_the_shade(ctx):
    """g_AO of the chain as SailorIblDesc.ao: radiance within the shade's 1e-4 relative bound of oracle.shade fed Ref32's plane"""
    f = synth.make_frame("tiny")
    W, H, N = f.cam.width, f.cam.height, len(f.lights)
    raw = synth.make_raw_depth(f.depth, f.cam.z_near)
    ext = ((W // 2, W // 2), (W // 2, W // 2), (W, H), (W, H))
    want_ao = Ref32.chain(f.cam.frame, raw, noise_texels(), ref.SHIPPED, ref.SHIPPED_BLUR, *ext)[3]
    assert is_lively(want_ao)
    ibl = synth.make_ibl_set(W, H, oracle.compute_brdf_lut(32, 32), with_ao=False)
    g, idx, _ = oracle.light_cull(f.cam.frame, W, H, f.lights, f.depth)
    oibl, _k = oracle.make_ibl(ibl.irradiance, ibl.env_chain, ibl.env_size, ibl.env_levels, ibl.brdf_lut, want_ao)
    want = oracle.shade(f.cam.frame, W, H, f.surface, f.lights, g, idx, None, ibl=oibl)
    no_ao, _k1 = oracle.make_ibl(ibl.irradiance, ibl.env_chain, ibl.env_size, ibl.env_levels, ibl.brdf_lut, None)
    assert not np.array_equal(want, oracle.shade(f.cam.frame, W, H, f.surface, f.lights, g, idx, None, ibl=no_ao)), "the AO plane changes the frame"

    hb = make_hbao(ctx, W, H)
    assert hb.extents == ext
    ao = hb.run(f.cam.frame, torch.from_numpy(raw).to(ctx.device))
    fp = ForwardPlus(ctx, W, H, N)
    lights = upload_lights(f.lights, ctx.device)
    fp.cull(f.cam.frame, lights, N, torch.from_numpy(f.depth).to(ctx.device))
    desc, keep = upload_ibl(ibl, ctx.device)
    desc.ao = ao.data_ptr()
    got = fp.shade(f.cam.frame, torch.from_numpy(f.surface).to(ctx.device), lights, N, None, ibl=desc).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.isfinite(got).all() and (err <= 1e-4 * np.abs(want.astype(np.float64))).all(), err.max()


def test_invalid_arguments_record_nothing(ctx):
    hb = make_hbao(ctx, 128, 96)
    cam, raw = raw_depth(128, 96)
    d = torch.from_numpy(raw).to(ctx.device)
    lib, hnd, p = ctx._lib, ctx.handle, lambda t: C.c_void_p(t.data_ptr())
    count = C.c_uint64()
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    before = count.value
    inv = _lib.load().sailor_hip_blit_nearest
    assert inv(hnd, None, 128, 96, p(hb.half_depth), 64, 64) == -1
    assert inv(hnd, p(d), 0, 96, p(hb.half_depth), 64, 64) == -1
    assert inv(hnd, p(d), 128, 96, p(hb.half_depth), 64, -1) == -1
    fr, P, B = C.byref(cam.frame), C.byref(hb.params), C.byref(hb.blur_params)
    assert lib.sailor_hip_hbao(hnd, fr, p(d), 128, 96, None, 16, 16, P, p(hb.ao), 64, 64) == -1
    assert lib.sailor_hip_hbao(hnd, fr, p(d), 128, 96, p(hb.noise), 16, 16, None, p(hb.ao), 64, 64) == -1
    assert lib.sailor_hip_hbao(hnd, None, p(d), 128, 96, p(hb.noise), 16, 16, P, p(hb.ao), 64, 64) == -1
    assert lib.sailor_hip_hbao(hnd, fr, p(d), 128, 96, p(hb.noise), 16, 0, P, p(hb.ao), 64, 64) == -1
    assert lib.sailor_hip_hbao_blur_pass(hnd, p(hb.ao), 64, 64, p(d), 128, 96, B, None, 128, 96, 1) == -1
    assert lib.sailor_hip_hbao_blur_pass(hnd, p(hb.ao), 64, 64, p(d), 128, 96, B, p(hb.ao), 64, 64, 1) == -1  # in place
    far = host.hbao_blur_params(radius=1000.0)
    assert lib.sailor_hip_hbao_blur_pass(hnd, p(hb.ao), 64, 64, p(d), 128, 96, C.byref(far), p(hb.temp), 128, 96, 1) == -1
    # the chain checks every argument before its first launch
    assert lib.sailor_hip_hbao_chain(hnd, fr, p(d), 128, 96, p(hb.half_depth), 64, 64, p(hb.noise), 16, 16, P, p(hb.ao), 64, 64, B, p(hb.temp), 128, 96,
                                     None, 128, 96) == -1
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    assert count.value == before
