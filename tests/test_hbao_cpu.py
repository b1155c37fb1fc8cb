"""CPU suite of the HBAO chain: registration and ABI, the parse of the shipped HBAO block, the NaN of screenSpace1Meter, the blit's index formula,
the two restatements of tests/hbao_ref.py held against each other, and the golden planes.  No GPU needed."""
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import hbao_ref as ref
from hbao_cases import OTHER, OTHER_BLUR, is_lively, noise_texels, raw_depth
from hbao_ref import Ref32, Ref64
from sailor_amd import _lib, host, runtime_binding, synth

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
SYMBOLS = ("sailor_hip_blit_nearest", "sailor_hip_hbao", "sailor_hip_hbao_blur_pass", "sailor_hip_hbao_chain")


def test_the_two_node_classes_are_registered():
    rt = runtime_binding.load()
    assert rt.sailor_rt_node_registered(b"PostProcess") == 1   # FrameGraph/PostProcessNode.cpp:19
    assert rt.sailor_rt_node_registered(b"Blit") == 1          # FrameGraph/BlitNode.cpp:18
    assert rt.sailor_rt_node_registered(b"Bloom") == 0 and rt.sailor_rt_node_registered(b"Clear") == 0


def test_abi_symbols_version_and_struct_layouts():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    declared = set(re.findall(r"\b(sailor_(?:hip|host)_\w+)\s*\(", header))
    lib = _lib.load()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.sailor_hip_version() >= 4
    import ctypes as C
    assert C.sizeof(_lib.HbaoParams) == 20 and C.sizeof(_lib.HbaoBlurParams) == 12   # std140 floats at 0, 4, 8, 12, 16 and 0, 4, 8
    p, b = host.hbao_params(), host.hbao_blur_params(radius=3)
    assert (p.occlusionRadius, p.occlusionPower, f32(p.occlusionAttenuation), f32(p.occlusionBias), p.noiseScale) == (700.0, 1.5, f32(0.1), f32(0.05), 25.0)
    assert (b.sharpness, b.distanceScale, b.radius) == (0.5, 2.0, 3.0)
    assert {k: v for k, v in ref.SHIPPED.items()} == _lib.HBAO_SHIPPED and ref.SHIPPED_BLUR == _lib.HBAO_BLUR_SHIPPED
    assert ref.shipped_extents(3840, 2160) == host.hbao_shipped_extents(3840, 2160) == ((1920, 1920), (1920, 1920), (3840, 3840), (3840, 3840))


def test_shipped_renderer_file_has_the_hbao_block_in_order():
    text = (ROOT / "tests" / "golden" / "DefaultRenderer.renderer").read_text()
    n, summary = runtime_binding.parse_renderer(text, 3840, 2160)
    nodes = summary[summary.index("nodes="):summary.index(";values=")]
    block = [
        "Blit[]{rt src=DepthBuffer;rt dst=HalfDepth;}",
        "DepthHighZ[]{rt src=HalfDepth;rt dst=DepthHighZ;}",
        "PostProcess[]{string defines=;string shader=Shaders/HBAO.shader;float data.noiseScale=25;float data.occlusionAttenuation=0.1;"
        "float data.occlusionBias=0.05;float data.occlusionPower=1.5;float data.occlusionRadius=700;rt color=AO;rt depthSampler=HalfDepth;"
        "rt noiseSampler=g_noiseSampler;}",
        "PostProcess[]{string defines=VERTICAL;string shader=Shaders/HBAO_Blur.shader;float data.distanceScale=2;float data.radius=5;"
        "float data.sharpness=0.5;rt color=TemporaryR8;rt aoSampler=AO;rt depthSampler=DepthBuffer;}",
        "PostProcess[]{string defines=HORIZONTAL;string shader=Shaders/HBAO_Blur.shader;float data.distanceScale=2;float data.radius=5;"
        "float data.sharpness=0.5;rt color=g_AO;rt aoSampler=TemporaryR8;rt depthSampler=DepthBuffer;}",
    ]
    assert ",".join(block) in nodes
    for target in ("HalfDepth:1920x1920:D32_SFLOAT_S8_UINT:1", "AO:1920x1920:R8_UNORM:1", "TemporaryR8:3840x3840:R8_UNORM:1", "g_AO:3840x3840:R8_UNORM:1"):
        assert target in summary, target
    assert "g_noiseSampler" in summary[summary.index(";samplers="):]


def test_noise_texture_is_the_16x16_rgba8_image():
    raw = np.load(ROOT / "tests" / "golden" / "hbao_noise.npy")
    assert raw.shape == (16, 16, 4) and raw.dtype == np.uint8 and len(np.unique(raw[..., :2])) > 4
    lin = noise_texels()
    assert lin.dtype == f32 and lin.shape == (16, 16, 4) and 0.0 <= lin.min() and lin.max() <= 1.0
    assert lin[0, 0, 0] == f32(((128 / 255 + 0.055) / 1.055) ** 2.4) and lin[0, 0, 3] == f32(raw[0, 0, 3] / 255)


@pytest.mark.parametrize("size", [(128, 96), (131, 77), (1920, 1080), (3840, 2160)])
def test_screen_space_one_meter_is_nan_for_the_synthetic_cameras(size):
    """HBAO.shader:211 in float32: projection * (0, 1, 0, 1) has w = 0 (a signed zero: -1 * 0 summed with zeros) and x = 0, x / w = 0 / 0 is NaN, so is the length, so is maxAORadius, and
    min(occlusionRadius, NaN) = "y < x ? y : x" is occlusionRadius"""
    cam = synth.make_camera(*size)
    P = np.array(list(cam.frame.projection), f32)   # column-major
    v = (f32(0.0), f32(1.0), f32(0.0), f32(1.0))
    res = [((P[0 + r] * v[0] + P[4 + r] * v[1]) + P[8 + r] * v[2]) + P[12 + r] * v[3] for r in range(4)]
    assert res[3] == 0 and res[0] == 0
    with np.errstate(all="ignore"):
        q = [x / res[3] for x in res]
        length = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        max_radius = (f32(100.0) - f32(cam.frame.cameraZNearZFar[0])) * length * f32(2.3)
    assert np.isnan(q[0]) and np.isnan(length) and np.isnan(max_radius)
    radius = f32(700.0)
    assert (max_radius if max_radius < radius else radius) == radius


@pytest.mark.parametrize("src,dst", [(7, 3), (131, 65), (77, 38), (96, 64), (128, 64), (5, 5), (3, 7), (1080, 960), (2, 1), (1, 1)])
def test_blit_index_is_the_texel_containing_the_destination_centre(src, dst):
    got = ref.blit_indices(src, dst)
    for i in range(dst):
        centre = Fraction(2 * i + 1, 2 * dst) * src   # the destination centre mapped into source texel units, exactly
        brute = [k for k in range(src) if k <= centre < k + 1]
        assert brute == [int(got[i])], (src, dst, i)
    plane = np.arange(src * 3, dtype=f32).reshape(3, src)
    np.testing.assert_array_equal(ref.blit(plane, dst, 3), plane[:, got])


CASES = {  # name -> (width, height, sky fraction, extents or None = shipped, parameters, blur parameters)
    "tiny": (128, 96, 0.0, None, ref.SHIPPED, ref.SHIPPED_BLUR),
    "ragged": (131, 77, 0.0, None, ref.SHIPPED, ref.SHIPPED_BLUR),
    "sky": (256, 144, 0.2, None, ref.SHIPPED, ref.SHIPPED_BLUR),
    "other": (128, 96, 0.0, ((64, 48), (50, 70), (128, 96), (128, 96)), OTHER, OTHER_BLUR),
}


def share_beyond_one_step(a, b):
    return float((np.abs(ref.codes(a).astype(np.int32) - ref.codes(b).astype(np.int32)) > 1).mean())


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_restatement_against_float64(name):
    """Ref32 (sinS = x, canonical exp2, fp32 order) against Ref64 (literal sin / acos, np.exp2) by 8-bit codes.  A threshold flip at HBAO.shader:135
    moves a single texel by many steps, so the condition is a share: per image at most 0.5 % of the texels differ by more than one step.
    Measured on these inputs, per pass on Ref32's own inputs and for the whole chain: 0 texels beyond one step in every image of every case
    (tiny 4 096 + 2 x 16 384 texels, ragged 4 225 + 2 x 17 161, sky 16 384 + 2 x 65 536, other 3 500 + 2 x 12 288), and no HBAO code differs at all.
    (The two do part on larger planes: a 320 x 320 AO plane of the 640 x 360 scene with sky blocks has 34 differing codes of 102 400, 13 of them -- 0.013 % --
    by more than one step, the largest by 19.)"""
    w, h, sky, ext, P, B = CASES[name]
    cam, raw = raw_depth(w, h, sky_fraction=sky)
    ext = ext or ref.shipped_extents(w, h)
    n = noise_texels()
    a = Ref32.chain(cam.frame, raw, n, P, B, *ext)
    assert is_lively(a[1]), "parity on a blank plane shows nothing"
    np.testing.assert_array_equal(a[0], Ref64.blit(raw, *ext[0]))
    per_pass = (Ref64.hbao(cam.frame, a[0], n, P, *ext[1]), Ref64.blur_pass(a[1], raw, B, *ext[2], True), Ref64.blur_pass(a[2], raw, B, *ext[3], False))
    chain = Ref64.chain(cam.frame, raw, n, P, B, *ext)[1:]
    shares = [share_beyond_one_step(x, y) for x, y in zip(a[1:], per_pass)] + [share_beyond_one_step(x, y) for x, y in zip(a[1:], chain)]
    print(name, "shares beyond one step (hbao, vertical, horizontal; per pass, then chain):", shares)
    assert max(shares) <= 0.005, shares
    for plane in a[1:]:
        assert plane.dtype == f32 and np.array_equal(plane, ref.codes(plane).astype(f32) / f32(255.0)), "an R8_UNORM plane holds k / 255"


def test_sky_and_small_radius_store_one():
    cam, raw = raw_depth(256, 144, sky_fraction=0.2)
    ao = Ref32.hbao(cam.frame, ref.blit(raw, 128, 128), noise_texels(), ref.SHIPPED, 128, 128)
    assert 0.05 < (ao == 1.0).mean() < 0.6
    far = Ref32.hbao(cam.frame, ref.blit(raw, 128, 128), noise_texels(), dict(ref.SHIPPED, occlusionRadius=1e-4), 128, 128)
    assert (far == 1.0).all(), "screenSpaceRadius < 1 everywhere (HBAO.shader:225)"


def test_golden_chain_of_the_tiny_frame():
    gold = np.load(ROOT / "tests" / "golden" / "tiny_hbao.npz")
    cam, raw = raw_depth(128, 96)
    half, ao, temp, g_ao = Ref32.chain(cam.frame, raw, noise_texels(), ref.SHIPPED, ref.SHIPPED_BLUR, *ref.shipped_extents(128, 96))
    np.testing.assert_array_equal(half.view(np.uint32), gold["half_depth_bits"])
    for name, plane in (("ao", ao), ("temp", temp), ("g_ao", g_ao)):
        assert gold[name].dtype == np.uint8
        np.testing.assert_array_equal(ref.codes(plane), gold[name])
