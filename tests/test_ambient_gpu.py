"""Ambient / image-based lighting term on the GPU: Standard.shader's AmbientLighting (:343-372) added to
the shaded radiance, and the ComputeBrdfLut.shader table it samples -- through the C-ABI, against the CPU oracle.
Tolerance as for K2: |gpu - ref| <= 1e-4*|ref|, no absolute floor (the samplers are bilinear fp32 on both sides)."""
import functools

import numpy as np
import pytest
import torch

import fuzz_cases
import ibl_cases
from oracle import oracle, oracle_f64
from sailor_amd import host, synth
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, compute_brdf_lut, upload_ibl, upload_lights, upload_shadow_maps

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 0.0


def close(got, ref):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bad = err > RTOL * np.abs(ref.astype(np.float64)) + ATOL
    assert np.isfinite(got).all() and not bad.any(), f"{bad.sum()} of {bad.size} out of tolerance, worst abs {err.max():.3e}"


def test_brdf_lut_matches_the_oracle(ctx):
    for w, h in ((32, 32), (48, 20)):
        got = compute_brdf_lut(ctx, w, h).cpu().numpy()
        ref = oracle.compute_brdf_lut(w, h)
        # 1 024-term sums of cos / sin / sqrt expressions: libm vs device trigonometry differ in the last ulp per term
        assert np.abs(got - ref).max() < 2e-6, np.abs(got - ref).max()
        assert 0.0 <= got.min() and got.max() <= 1.0 + 1e-6
        assert got[0, 0, 1] > 0.99 and got[h - 1, w - 1, 0] < 0.5  # grazing + smooth: all Fresnel; normal + rough: darkened


@pytest.mark.parametrize("name", ["tiny", "tiny_csm"])
@pytest.mark.parametrize("with_ao", [True, False])
def test_ambient_plus_lights(ctx, name, with_ao):
    f = synth.make_frame(name)
    W, H, N = f.cam.width, f.cam.height, len(f.lights)
    ibl = synth.make_ibl_set(W, H, oracle.compute_brdf_lut(32, 32), with_ao=with_ao)
    g, idx, _ = oracle.light_cull(f.cam.frame, W, H, f.lights, f.depth)
    ocsm = None
    if f.shadows is not None:
        ocsm, _k = oracle.make_csm(f.shadows.lights_matrices, f.shadows.maps)
    oibl, _k2 = oracle.make_ibl(ibl.irradiance, ibl.env_chain, ibl.env_size, ibl.env_levels, ibl.brdf_lut, ibl.ao)
    ref = oracle.shade(f.cam.frame, W, H, f.surface, f.lights, g, idx, ocsm, ibl=oibl)
    direct = oracle.shade(f.cam.frame, W, H, f.surface, f.lights, g, idx, ocsm)
    assert (ref[..., :3] - direct[..., :3]).min() > 0.0, "the ambient term is strictly positive on this sky"

    fp = ForwardPlus(ctx, W, H, N)
    lights = upload_lights(f.lights, ctx.device)
    fp.cull(f.cam.frame, lights, N, torch.from_numpy(f.depth).to(ctx.device))
    csm, keep = upload_shadow_maps(f.shadows, ctx.device) if f.shadows is not None else (None, None)
    desc, keep2 = upload_ibl(ibl, ctx.device)
    got = fp.shade(f.cam.frame, torch.from_numpy(f.surface).to(ctx.device), lights, N, csm, ibl=desc).cpu().numpy()
    close(got, ref)
    np.testing.assert_array_equal(got[..., 3], ref[..., 3])


def test_ambient_on_bands_and_ragged_viewport(ctx):
    """AO rows follow the band; 131x77 has partial tiles."""
    w, h = 131, 77
    cam = synth.make_camera(w, h)
    depth = synth.make_linear_depth(w, h, 5)
    lights = synth.make_lights(cam, depth, synth.LightSetConfig(count=300, radius_scale=5.0, spot_fraction=0.3), 5)
    surface = synth.make_surface(cam, depth, 5)
    ibl = synth.make_ibl_set(w, h, oracle.compute_brdf_lut(16, 16), env_size=32, irr_size=8, seed=5)
    g, idx, _ = oracle.light_cull(cam.frame, w, h, lights, depth)
    oibl, _k = oracle.make_ibl(ibl.irradiance, ibl.env_chain, ibl.env_size, ibl.env_levels, ibl.brdf_lut, ibl.ao)
    ref = oracle.shade(cam.frame, w, h, surface, lights, g, idx, ibl=oibl)
    d_lights = upload_lights(lights, ctx.device)
    for r in range(2):
        band = host.band_for_rank(w, h, r, 2)
        rows = slice(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)
        fp = ForwardPlus(ctx, w, h, len(lights), band=band)
        fp.cull(cam.frame, d_lights, len(lights), torch.from_numpy(np.ascontiguousarray(depth[rows])).to(ctx.device))
        desc, keep = upload_ibl(ibl, ctx.device, ao_rows=(rows.start, rows.stop))
        got = fp.shade(cam.frame, torch.from_numpy(np.ascontiguousarray(surface[:, rows])).to(ctx.device), d_lights, len(lights), None, ibl=desc).cpu().numpy()
        close(got, ref[rows])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The ambient term against the float64 restatement (oracle/oracle_f64.py: written from the shader text and the Vulkan sampling rules, sharing
# nothing with the C oracle's sampler), on tests/ibl_cases.py's edge inputs; every shade variant that carries the term; hostile inputs by class.
# ---------------------------------------------------------------------------------------------------------------------------------------------
FORMS = {"": (False, False), "_p": (False, True), "_t": (True, False), "_pt": (True, True)}   # suffix -> (the cull's tile lists, prepared lights)


def gpu_shade(ctx, cam, depth, surface, lights, ibl_set, form, shadows=None, band=None):
    """cull + shade of one band through one of the four entry forms -> (radiance, launched kernel names, framebuffer rows)"""
    W, H, N = cam.width, cam.height, len(lights)
    tile_lists, prep = FORMS[form]
    l = upload_lights(lights, ctx.device)
    fp = ForwardPlus(ctx, W, H, max(N, 1), band=band, prepared=PreparedLights(ctx, l, N) if prep else None)
    fp.shade_from_tile_lists = tile_lists
    rows = slice(fp.band.fbRowBegin, fp.band.fbRowBegin + fp.band.fbRowCount)
    fp.cull(cam.frame, l, N, torch.from_numpy(np.ascontiguousarray(depth[rows])).to(ctx.device))
    desc, keep = ibl_cases.upload_guarded(ibl_set, ctx.device, ao_rows=(rows.start, rows.stop))
    csm, keep2 = upload_shadow_maps(shadows, ctx.device) if shadows is not None else (None, None)
    s = torch.from_numpy(np.ascontiguousarray(surface[:, rows])).to(ctx.device)
    out = []
    names = ctx.launches_of(lambda: out.append(fp.shade(cam.frame, s, l, N, csm, ibl=desc)))
    ctx.synchronize()
    return out[0].cpu().numpy(), names, rows


def c_oracle_shade(cam, depth, surface, lights, ibl_set, shadows=None):
    W, H = cam.width, cam.height
    g, idx, _ = oracle.light_cull(cam.frame, W, H, lights, depth)
    ocsm = oracle.make_csm(shadows.lights_matrices, shadows.maps)[0] if shadows is not None else None
    oibl, _k = oracle.make_ibl(ibl_set.irradiance, ibl_set.env_chain, ibl_set.env_size, ibl_set.env_levels, ibl_set.brdf_lut, ibl_set.ao)
    return oracle.shade(cam.frame, W, H, surface, lights, g, idx, ocsm, ibl=oibl), g, idx


@functools.lru_cache(maxsize=None)
def edge_reference(tex, size):
    """(edge surface, texture set, float64 radiance, left-out mask, C oracle radiance) -- computed once per (set, size)"""
    W, H = size
    e = ibl_cases.make_edge_surface(W, H, ibl_cases.TEXTURE_SETS[tex][1])
    ts = ibl_cases.make_texture_set(tex, W, H)
    c_ref, g, idx = c_oracle_shade(e.cam, e.depth, e.surface, e.lights, ts)
    ref, m_n, m_lr = oracle_f64.shade(bytes(e.cam.frame), W, H, e.surface, e.lights, g, idx, None, ibl=ibl_cases.as_f64_ibl(ts), want_seam_margin=True)
    return e, ts, ref, ibl_cases.left_out(e, m_n, m_lr), c_ref


def k2_excess(got, ref):
    """err / tol per pixel under the project's K2 bound |got - f64| <= 1e-4 |f64| + 1e-7 max|f64|"""
    err = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
    return (err / (1e-4 * np.abs(ref[..., :3]) + 1e-7 * np.abs(ref[..., :3]).max())).max(-1)


@pytest.mark.parametrize("size", ibl_cases.SIZES)
@pytest.mark.parametrize("tex", list(ibl_cases.TEXTURE_SETS))
def test_ambient_edges_against_float64(ctx, tex, size):
    """Every texture set on the edge surface under 64 point and spot lights: the K2 bound against float64 on every pixel but those whose cube
    direction a fp32 evaluation may put on the other face (a condition on the inputs -- ibl_cases.left_out: Lr within 1e-4 of a seam, or a random
    normal strictly between 0 and 1e-4 of one; at most 1 % of the pixels; never an exact-tie pixel), alpha bit for bit.  The C oracle meets the same
    bound on the same inputs (tests/test_oracle_cpu.py); measured: C oracle worst err / tol 0.21, kernel see DESIGN.md section 2."""
    e, ts, ref, out, c_ref = edge_reference(tex, size)
    assert out.sum() <= 0.01 * out.size and not (out & e.exact_tie).any()
    form = "_pt" if size[0] == 40 else ""
    got, names, _rows = gpu_shade(ctx, e.cam, e.depth, e.surface, e.lights, ts, form)
    assert names == ["k2_shade_ibl" + form], names
    excess = k2_excess(got, ref)
    print(f"[ambient f64] edge {size[0]}x{size[1]} set {tex}: kernel worst err / tol {excess[~out].max():.3f} (C oracle {k2_excess(c_ref, ref)[~out].max():.3f}), "
          f"{out.sum()} pixels left out")
    assert np.isfinite(got).all()
    assert (excess[~out] <= 1.0).all(), f"{(excess[~out] > 1.0).sum()} pixels beyond the K2 bound, first {np.argwhere((excess > 1.0) & ~out)[:5].tolist()}"
    np.testing.assert_array_equal(got[..., 3], ref[..., 3].astype(np.float32))


@functools.lru_cache(maxsize=None)
def variant_config(name):
    """(cam, depth, surface, lights, texture set, shadow set or None, C oracle radiance)"""
    if name == "ibl":
        e = ibl_cases.make_edge_surface(40, 24, 4)
        cfg = (e.cam, e.depth, e.surface, e.lights, ibl_cases.make_texture_set("b", 40, 24), None)
    else:
        f = synth.make_frame("tiny_csm")
        cfg = (f.cam, f.depth, f.surface, f.lights, ibl_cases.make_texture_set("d", f.cam.width, f.cam.height), f.shadows)
    return cfg + (c_oracle_shade(*cfg)[0],)


@pytest.mark.parametrize("name", ["ibl", "csm_ibl"])
def test_every_shade_variant_with_the_ambient_term(ctx, name):
    """k2_shade_ibl and k2_shade_csm_ibl (tiny_csm's maps) through their four entry forms -- canonical lists or the cull's tile lists, 112-byte records
    or prepared lights -- on the whole frame and on two bands cut at an odd tile row (the AO rows follow the band): each run launches the kernel it is
    meant to, holds the C oracle to 1e-4 relative with no floor, and the four forms of one configuration are equal bit for bit (same lists, same
    arithmetic)."""
    cam, depth, surface, lights, ts, shadows, ref = variant_config(name)
    W, H = cam.width, cam.height
    Ty = host.num_tiles(W, H)[1]
    cut = Ty // 2 if (Ty // 2) % 2 == 1 else Ty // 2 + 1
    assert 0 < cut < Ty and cut % 2 == 1
    for band in (None, (0, cut), (cut, Ty)):
        first = None
        for form in FORMS:
            b = host.band_from_tile_rows(W, H, *band) if band is not None else None
            got, names, rows = gpu_shade(ctx, cam, depth, surface, lights, ts, form, shadows, b)
            assert names == [f"k2_shade_{name}{form}"], (band, form, names)
            assert got.shape[0] == rows.stop - rows.start
            err = np.abs(got.astype(np.float64) - ref[rows])
            assert np.isfinite(got).all() and (err <= RTOL * np.abs(ref[rows].astype(np.float64))).all(), (band, form, float(err.max()))
            if first is None:
                first = got
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), f"band {band}: form '{form}' differs from form '' in {(got != first).sum()} values"


@pytest.mark.parametrize("size", ibl_cases.SIZES)
@pytest.mark.parametrize("tex", ["b", "d"])
def test_hostile_ambient_inputs_by_class(ctx, tex, size):
    """NaN and all-zero normals, infinite positions, NaN / infinite / negative roughness and AO, an infinite metallic, one infinite and one NaN env
    texel: the non-finite results are the oracle's BY CLASS (NaN, +Inf, -Inf), the finite ones within 1e-4.  A NaN or infinite texture coordinate
    reaches float -> int conversions, which the oracle defines as the device's saturating convert does (see sampling.h)."""
    W, H = size
    e = ibl_cases.make_edge_surface(W, H, ibl_cases.TEXTURE_SETS[tex][1], hostile=True)
    ts = ibl_cases.make_texture_set(tex, W, H, hostile=True)
    ref, _g, _i = c_oracle_shade(e.cam, e.depth, e.surface, e.lights, ts)
    assert not np.isfinite(ref).all() and np.isfinite(ref).mean() > 0.9
    for form in ("_pt", ""):
        got, names, _rows = gpu_shade(ctx, e.cam, e.depth, e.surface, e.lights, ts, form)
        mism = fuzz_cases.nonfinite_mismatch(got, ref)
        assert mism is None, f"form '{form}': the {mism[0]} masks differ at {len(mism[1])} values, first {mism[1][0].tolist()}: got {got[tuple(mism[1][0][:2])]} " \
                             f"ref {ref[tuple(mism[1][0][:2])]} surface {e.surface[:, mism[1][0][0], mism[1][0][1]].tolist()}"
        fin = np.isfinite(ref)
        err = fuzz_cases.finite_abs_diff(got, ref, fin)
        assert (err[fin] <= RTOL * np.abs(ref.astype(np.float64))[fin]).all(), (form, float(err.max()))


@pytest.mark.parametrize("size", [(32, 32), (48, 20), (1, 1)])
def test_brdf_lut_against_float64(ctx, size):
    """k_brdf_lut against oracle_f64.brdf_lut.  The C oracle's worst absolute error against float64 is measured here, per size (1.5e-3, 1.0e-3 and
    1.1e-5: SampleGGX's `alpha^2 - 1` in fp32 at small roughness, tests/test_oracle_cpu.py); the kernel's may be at most twice that -- both are fp32
    evaluations of the same 1 024-term sums, the factor covers libm against device trigonometry -- and it stays within 2e-6 of the C oracle."""
    w, h = size
    ref = oracle_f64.brdf_lut(w, h)
    c = oracle.compute_brdf_lut(w, h)
    got = compute_brdf_lut(ctx, w, h).cpu().numpy()
    c_err, k_err = np.abs(c - ref).max(), np.abs(got - ref).max()
    print(f"[brdf lut f64] {w}x{h}: worst abs error C oracle {c_err:.3e}, kernel {k_err:.3e}, kernel against C oracle {np.abs(got - c).max():.3e}")
    assert np.isfinite(got).all() and k_err <= 2.0 * c_err, (k_err, c_err)
    assert np.abs(got - c).max() < 2e-6
