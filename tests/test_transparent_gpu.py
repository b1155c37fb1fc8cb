"""The Transparent render queue (sailor_amd/csrc/surface_transparent.hip) through the C-ABI and SurfacePass.transparent against tests/transparent_ref.py:
(a) every layer of every case of tests/transparent_cases.py bit for bit -- last, coverage, the committed count, the three planes, emissive and aoOut; (b) the
blend alone on arbitrary and hostile planes in every mode; (c) the pass end to end through the real shade against the float64 chain; (d) a layer budget below
and at the depth of deep_5 and its overflow; (e) two bands; (f) the recorded form captured into a graph; the refusals; the launch times at 3840 x 2160."""
import ctypes as C

import numpy as np
import pytest
import torch

import surface_ref as ref
import transparent_cases as cases
import transparent_ref as tr
from sailor_amd import _lib, host
from sailor_amd.forward_plus import ForwardPlus, HipContext, SurfacePass, linearize_depth, upload_lights
from test_gltf_gpu import Uploaded
from test_surface_gpu import dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def restated(scenes):
    """name -> (depth attachment, layers): computed once, shared, left unchanged"""
    out = {}
    for name, s in scenes.items():
        depth = cases.depth_attachment(s)
        out[name] = (depth, tr.layers(s, depth)[0])
    return out


def albedo_as_radiance(surface, ao):
    """a substitute for the shade, a pure function of the pixel's planes: radiance = (albedo.rgb, metallic)"""
    return surface[2].contiguous()


def albedo_np(planes, ao):
    return planes[2]


def run(ctx, s, depth, shade, target, layers=None, band=None, up=None, on_layer=None):
    """the scene through SurfacePass.transparent -> (the band's rows of the target, the counters, the pass); on_layer gets the pass in front of its arguments"""
    up = up or Uploaded(ctx, s)
    draws = [dict(d, blend=sd["blend"]) for d, sd in zip(up.draws, s["draws"])]
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=len(draws))
    rows = slice(sp.band.fbRowBegin, sp.band.fbRowBegin + sp.band.fbRowCount)
    t = dev(ctx, target[rows])
    counts = sp.transparent(s["cam"].frame, draws, up.instances, up.materials, up.textures, up.num_textures, dev(ctx, depth), shade, t, layers=layers,
                            prim_base=s.get("prim_base", 0), on_layer=None if on_layer is None else (lambda *a: on_layer(sp, *a)))
    ctx.synchronize()
    return t.cpu().numpy(), counts.cpu().numpy(), sp


def same(got, want):
    return ref.same_bits_or_class(np.asarray(got), np.asarray(want)).all()


# ---- (a) every layer ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_layer_of_every_case_against_the_restatement(ctx, scenes, restated, name):
    s = scenes[name]
    depth, L = restated[name]
    seen = []

    def on_layer(sp, k, surface, cov, emissive, ao):
        ctx.synchronize()
        seen.append(dict(planes=surface.cpu().numpy(), covered=cov.cpu().numpy().astype(bool), emissive=None if emissive is None else emissive.cpu().numpy(),
                         ao=None if ao is None else ao.cpu().numpy(), last=sp.last.cpu().numpy().view(np.uint32), keys=sp.download_keys()))
    _, counts, sp = run(ctx, s, depth, albedo_as_radiance, cases.target_of(s), on_layer=on_layer)
    assert len(seen) == len(L) and counts.tolist() == [int(l["covered"].sum()) for l in L] + [0], (counts.tolist(), len(L))
    d_bits = depth.view(np.uint32)
    last = np.zeros((s["H"], s["W"]), np.uint32)
    for k, (got, want) in enumerate(zip(seen, L)):
        last = np.where(want["covered"], want["last"], last)   # the plane keeps the order a pixel committed LAST: a pixel without a k-th fragment keeps its own
        np.testing.assert_array_equal(got["last"], last, err_msg=f"{name} layer {k}: last")
        np.testing.assert_array_equal(got["covered"], want["covered"], err_msg=f"{name} layer {k}: coverage")
        np.testing.assert_array_equal(got["keys"], (want["z"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | want["last"], err_msg=f"{name} layer {k}: keys")
        assert (want["z"].view(np.uint32)[want["covered"]] >= d_bits[want["covered"]]).all()
        assert same(got["planes"], want["planes"]), f"{name} layer {k}: planes"
        if got["emissive"] is not None:
            assert same(got["emissive"], want["emissive"]) and same(got["ao"], want["ao_out"]), f"{name} layer {k}: emissive / aoOut"
        else:
            assert (want["emissive"] == tr.gltf_ref.NO_EMISSIVE).all()


# ---- (b) the blend alone --------------------------------------------------------------------------------------------------------------------------------
def test_the_blend_alone_in_every_mode_on_arbitrary_and_hostile_planes(ctx, scenes, restated):
    """layer 0 of mixed_modes holds pixels of all three modes (layers=0 records the overflow round alone, which commits it); radiance, P0 and emissive are
    arbitrary, with 0, values beyond 1, negative values, NaN and Inf among the alphas and the colours"""
    s = scenes["mixed_modes"]
    depth, L = restated["mixed_modes"]
    W, H = s["W"], s["H"]
    _, counts, sp = run(ctx, s, depth, albedo_as_radiance, cases.target_of(s), layers=0)
    l0 = L[0]
    assert counts.tolist() == [int(l0["covered"].sum())] and set(np.unique(l0["blend"][l0["covered"]])) == {tr.NONE, tr.ADDITIVE, tr.ALPHA}
    rng = np.random.default_rng(11)
    rad, p0, em, tgt = (rng.uniform(-2, 4, (H, W, 4)).astype(np.float32) for _ in range(4))
    hostile = np.array([0.0, -0.0, 1.0, 1.5, -3.0, np.nan, np.inf, -np.inf, 1e-40, 3e38], np.float32)
    p0[..., 3] = np.where(rng.uniform(size=(H, W)) < 0.5, hostile[rng.integers(0, len(hostile), (H, W))], p0[..., 3])
    for a in (rad, em, tgt):
        at = rng.uniform(size=a.shape) < 0.05
        a[at] = hostile[rng.integers(0, len(hostile), int(at.sum()))]
    c = l0["covered"]
    for with_emissive in (True, False):
        t, d_rad, d_p0, d_em = dev(ctx, tgt), dev(ctx, rad), dev(ctx, p0), dev(ctx, em)
        _lib.check(ctx._lib.sailor_hip_surface_blend(ctx.handle, d_rad.data_ptr(), d_p0.data_ptr(), d_em.data_ptr() if with_emissive else None,
                                                     sp.workspace.data_ptr(), sp.workspace.numel(), t.data_ptr(), W, H, C.byref(sp.band)), "sailor_hip_surface_blend", ctx.handle)
        ctx.synchronize()
        got = t.cpu().numpy()
        with np.errstate(all="ignore"):
            src = np.concatenate([em[..., :3] + rad[..., :3] if with_emissive else rad[..., :3], p0[..., 3:4]], -1)
        want = tr.blend(l0["blend"][c], src[c], tgt[c])
        for mode in (tr.NONE, tr.ADDITIVE, tr.ALPHA):
            m = l0["blend"][c] == mode
            assert m.sum() > 50 and same(got[c][m], want[m]), (with_emissive, mode)
            assert np.isnan(want[m]).any() and np.isinf(want[m]).any() and np.isfinite(want[m]).any()
        np.testing.assert_array_equal(got[~c].view(np.uint32), tgt[~c].view(np.uint32))


# ---- (c) end to end through the real shade --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_pass_through_the_real_shade_against_the_float64_chain(ctx, scenes, restated, name):
    """the final target against the float64 chain (restatement's planes -> oracle_f64.shade -> float64 blend) under the shade's per-layer bound
    1e-4 |f64| + 1e-7 max |f64| propagated through the blend weights, plus 4 x the measured error of the fp32 restatement chain
    (tests/transparent_cases.py CHAIN_ERROR; tests/test_transparent_cpu.py measures it) -- the margin tests/test_ui_gpu.py uses for blend chains.  No pixel is
    left out: both chains shade the restatement's fp32 planes, so no texture fetch can pick another texel.  Non-finite channels are compared by class."""
    s = scenes[name]
    depth, L = restated[name]
    W, H, lights = s["W"], s["H"], s["lights"]
    cam = s["cam"]
    d_depth = dev(ctx, depth)
    fp = ForwardPlus(ctx, W, H, len(lights))
    d_lights = upload_lights(lights, ctx.device)
    fp.cull(cam.frame, d_lights, len(lights), linearize_depth(ctx, cam.frame, d_depth))
    tgt = cases.target_of(s)
    got, counts, _ = run(ctx, s, depth, lambda surface, ao: fp.shade(cam.frame, surface, d_lights, len(lights)), tgt)
    assert len(counts) == len(L) + 1
    s64 = cases.shaders(s, depth)[1]
    c64 = tr.composite(L, s64, tgt, np.float64)
    tol = cases.chain_tolerance(L, s64, tgt, 4 * cases.CHAIN_ERROR)
    touched = L[0]["covered"]
    finite = np.isfinite(c64)
    assert (np.isnan(got) == np.isnan(c64)).all() and (np.isinf(got) == np.isinf(c64)).all(), "non-finite channels differ in class"
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - c64)
    check = touched[..., None] & finite
    print(f"[{name}] worst err {err[check].max():.3e}, worst err / tol {(err[check] / tol[check]).max():.3f} over {int(check.sum())} channels of {int(touched.sum())} pixels")
    assert (err[check] <= tol[check]).all(), f"{int((err > tol)[check].sum())} channels beyond the bound"
    np.testing.assert_array_equal(got[~touched].view(np.uint32), tgt[~touched].view(np.uint32))
    lit = np.concatenate([s64(l["planes"], None)[l["covered"]][:, :3].ravel() for l in L])
    assert lit.max() > 0.05, "the layers are lit"


# ---- (d) the layer budget ---------------------------------------------------------------------------------------------------------------------------------
def test_a_layer_budget_below_and_at_the_depth_of_deep_5(ctx, scenes, restated):
    s = scenes["deep_5"]
    depth, L = restated["deep_5"]
    tgt, up = cases.target_of(s), Uploaded(ctx, s)
    px = s["W"] * s["H"]
    three, counts3, _ = run(ctx, s, depth, albedo_as_radiance, tgt, layers=3, up=up)
    assert counts3.tolist() == [px, px, px, px], "three layers and an overflow of every pixel"
    assert same(three, tr.composite(L, albedo_np, tgt, limit=3))
    five, counts5, _ = run(ctx, s, depth, albedo_as_radiance, tgt, layers=5, up=up)
    unbounded, counts, _ = run(ctx, s, depth, albedo_as_radiance, tgt, up=up)
    assert counts5.tolist() == [px] * 5 + [0] and counts.tolist() == counts5.tolist()
    np.testing.assert_array_equal(five.view(np.uint32), unbounded.view(np.uint32))
    assert same(five, tr.composite(L, albedo_np, tgt)) and not same(five, three)


# ---- (e) bands ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["order_abc", "cutout_gltf", "near_cut"])
def test_two_bands_give_the_whole_frames_bits(ctx, scenes, restated, name):
    s = scenes[name]
    depth, L = restated[name]
    tgt, up = cases.target_of(s), Uploaded(ctx, s)
    whole, counts, sp = run(ctx, s, depth, albedo_as_radiance, tgt, up=up)
    assert same(whole, tr.composite(L, albedo_np, tgt))
    parts, lasts, totals = [], [], 0
    for rank in reversed(range(2)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
        band = host.band_for_rank(s["W"], s["H"], rank, 2)
        got, c, p = run(ctx, s, depth, albedo_as_radiance, tgt, band=band, up=up)
        assert 0 < band.fbRowCount < s["H"]
        parts.append(got)
        lasts.append(p.last.cpu().numpy())
        totals += int(c.sum())
    np.testing.assert_array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    np.testing.assert_array_equal(np.concatenate(lasts), sp.last.cpu().numpy())
    assert totals == int(counts.sum())


# ---- (f) the recorded form in a graph -------------------------------------------------------------------------------------------------------------------
def test_the_recorded_form_captured_into_a_graph_and_replayed(ctx, scenes, restated):
    s = scenes["mixed_modes"]
    depth, L = restated["mixed_modes"]
    tgt = cases.target_of(s)
    eager, eager_counts, _ = run(ctx, s, depth, albedo_as_radiance, tgt, layers=2)
    assert same(eager, tr.composite(L, albedo_np, tgt, limit=2)) and eager_counts[2] == int(L[2]["covered"].sum()) > 0
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        up = Uploaded(c2, s)
        draws = [dict(d, blend=sd["blend"]) for d, sd in zip(up.draws, s["draws"])]
        sp = SurfacePass(c2, s["W"], s["H"], max_draws=len(draws))
        seed, work, d_depth = dev(ctx, tgt), dev(ctx, np.zeros_like(tgt)), dev(ctx, depth)
        out = torch.zeros(3, dtype=torch.int32, device=ctx.device)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            work.copy_(seed)      # the pass rewrites its target in place: every replay starts from the seed
            out.copy_(sp.transparent(s["cam"].frame, draws, up.instances, up.materials, up.textures, up.num_textures, d_depth, albedo_as_radiance, work, layers=2))
        for _ in range(2):
            work.fill_(7.0)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(work.cpu().numpy().view(np.uint32), eager.view(np.uint32))
            assert out.cpu().numpy().tolist() == eager_counts.tolist()
    finally:
        c2.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_say_why(ctx, scenes):
    lib = ctx._lib
    s = scenes["cutout_gltf"]
    W, H = s["W"], s["H"]
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, W, H, max_draws=2)
    ws, n, band, frame = sp.workspace.data_ptr(), sp.workspace.numel(), sp.band, s["cam"].frame
    bad_band = _lib.Band(0, 1, 3, 16)
    last = torch.zeros((H, W), dtype=torch.int32, device=ctx.device)
    depth = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
    plane = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    count = torch.zeros(2, dtype=torch.int32, device=ctx.device)
    CUT, GLTF, CULL, SHIFT = _lib.SURFACE_ALPHA_CUTOUT, _lib.SURFACE_GLTF, _lib.SURFACE_CULL_BACK, _lib.SURFACE_BLEND_SHIFT
    ALPHA, MULTIPLY = _lib.SURFACE_BLEND_ALPHA << SHIFT, _lib.SURFACE_BLEND_MULTIPLY << SHIFT
    d = up.draws[1]

    def desc(flags, prim_base=0, vertices=d["vertices"].data_ptr()):
        return _lib.SurfaceDraw(vertices, d["indices"].data_ptr(), d["instance_ids"].data_ptr(), 2, 1, prim_base, flags, 0, 0)

    def peel(dd, entry=lib.sailor_hip_surface_peel_draw, index=0, workspace=ws, size=n, b=band, mats=up.materials.data_ptr(), z=depth.data_ptr(), l=last.data_ptr()):
        return lambda: entry(ctx.handle, C.byref(frame), C.byref(dd), up.instances.data_ptr(), mats, 3, up.textures.data_ptr(), up.num_textures, index, W, H, C.byref(b),
                             workspace, size, z, l)

    def old(dd, entry):
        return lambda: entry(ctx.handle, C.byref(frame), C.byref(dd), up.instances.data_ptr(), up.materials.data_ptr(), 3, up.textures.data_ptr(), up.num_textures, 0, W, H,
                             C.byref(band), ws, n)
    gl = lib.sailor_hip_surface_peel_draw_gltf
    invalid = {
        "peel_begin: invalid band": lambda: lib.sailor_hip_surface_peel_begin(ctx.handle, W, H, C.byref(bad_band), ws, n, last.data_ptr(), 1),
        "peel_begin: null workspace": lambda: lib.sailor_hip_surface_peel_begin(ctx.handle, W, H, C.byref(band), None, n, last.data_ptr(), 1),
        "peel_begin: workspace too small": lambda: lib.sailor_hip_surface_peel_begin(ctx.handle, W, H, C.byref(band), ws, 1000, last.data_ptr(), 1),
        "peel_begin: null last": lambda: lib.sailor_hip_surface_peel_begin(ctx.handle, W, H, C.byref(band), ws, n, None, 1),
        "peel_begin: misaligned last": lambda: lib.sailor_hip_surface_peel_begin(ctx.handle, W, H, C.byref(band), ws, n, last.data_ptr() + 2, 0),
        "peel_draw: unknown flag bits": peel(desc(ALPHA | 32)),
        "peel_draw: the glTF flag": peel(desc(ALPHA | GLTF)),
        "peel_draw: cutout without materials": peel(desc(ALPHA | CUT), mats=None),
        "peel_draw: null depth": peel(desc(ALPHA), z=None),
        "peel_draw: misaligned depth": peel(desc(ALPHA), z=depth.data_ptr() + 2),
        "peel_draw: null last": peel(desc(ALPHA), l=None),
        "peel_draw: null vertices": peel(desc(ALPHA, vertices=None)),
        "peel_draw: drawIndex >= maxDraws": peel(desc(ALPHA), index=2),
        "peel_draw: primBase overflow": peel(desc(ALPHA, prim_base=2 ** 32 - 1 - 4)),
        "peel_draw: invalid band": peel(desc(ALPHA), b=bad_band),
        "peel_draw: workspace too small": peel(desc(ALPHA), size=1000),
        "peel_draw_gltf: without the glTF flag": peel(desc(ALPHA | CUT), entry=gl),
        "peel_draw_gltf: unknown flag bits": peel(desc(GLTF | ALPHA | 64), entry=gl),
        "peel_draw_gltf: null last": peel(desc(GLTF | ALPHA), entry=gl, l=None),
        "peel_commit: invalid band": lambda: lib.sailor_hip_surface_peel_commit(ctx.handle, W, H, C.byref(bad_band), ws, n, last.data_ptr(), count.data_ptr()),
        "peel_commit: null last": lambda: lib.sailor_hip_surface_peel_commit(ctx.handle, W, H, C.byref(band), ws, n, None, count.data_ptr()),
        "peel_commit: null counter": lambda: lib.sailor_hip_surface_peel_commit(ctx.handle, W, H, C.byref(band), ws, n, last.data_ptr(), None),
        "peel_commit: misaligned counter": lambda: lib.sailor_hip_surface_peel_commit(ctx.handle, W, H, C.byref(band), ws, n, last.data_ptr(), count.data_ptr() + 2),
        "blend: null radiance": lambda: lib.sailor_hip_surface_blend(ctx.handle, None, plane.data_ptr(), None, ws, n, plane.data_ptr(), W, H, C.byref(band)),
        "blend: null P0": lambda: lib.sailor_hip_surface_blend(ctx.handle, plane.data_ptr(), None, None, ws, n, plane.data_ptr(), W, H, C.byref(band)),
        "blend: null target": lambda: lib.sailor_hip_surface_blend(ctx.handle, plane.data_ptr(), plane.data_ptr(), None, ws, n, None, W, H, C.byref(band)),
        "blend: misaligned emissive": lambda: lib.sailor_hip_surface_blend(ctx.handle, plane.data_ptr(), plane.data_ptr(), plane.data_ptr() + 4, ws, n, plane.data_ptr(), W, H,
                                                                           C.byref(band)),
        "blend: workspace too small": lambda: lib.sailor_hip_surface_blend(ctx.handle, plane.data_ptr(), plane.data_ptr(), None, ws, 1000, plane.data_ptr(), W, H, C.byref(band)),
        "blend: invalid band": lambda: lib.sailor_hip_surface_blend(ctx.handle, plane.data_ptr(), plane.data_ptr(), None, ws, n, plane.data_ptr(), W, H, C.byref(bad_band)),
    }
    # the existing draw entries keep refusing the new bits, every mode of the field
    for mode in (1, 2, 3):
        invalid[f"draw_masked: blend mode {mode}"] = old(desc(CUT | (mode << SHIFT)), lib.sailor_hip_surface_draw_masked)
        invalid[f"draw_gltf: blend mode {mode}"] = old(desc(GLTF | (mode << SHIFT)), lib.sailor_hip_surface_draw_gltf)
        invalid[f"draw_lod: blend mode {mode}"] = old(desc(mode << SHIFT), lib.sailor_hip_surface_draw_lod)
        invalid[f"draw: blend mode {mode}"] = (lambda dd: lambda: lib.sailor_hip_surface_draw(ctx.handle, C.byref(frame), C.byref(dd), up.instances.data_ptr(), 0, W, H,
                                                                                              C.byref(band), ws, n))(desc(mode << SHIFT))
    unsupported = {"peel_draw: Multiply": peel(desc(MULTIPLY)), "peel_draw_gltf: Multiply": peel(desc(GLTF | MULTIPLY | CUT), entry=gl)}
    for status, calls in ((-1, invalid), (-7, unsupported)):
        for what, call in calls.items():
            before, _ = ctx.launch_log(0)
            assert call() == status, what
            after, _ = ctx.launch_log(0)
            assert after == before, f"{what}: launched {after - before} kernels"
            assert b"sailor_hip_surface_" in lib.sailor_hip_context_last_error(ctx.handle), what
    last_error = lambda call: (call(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"peel_draw: unknown flags" in last_error(peel(desc(ALPHA | 32))) and b"draw_masked: unknown flags" in last_error(old(desc(CUT | ALPHA), lib.sailor_hip_surface_draw_masked))
    assert b"Multiply" in last_error(peel(desc(MULTIPLY))) and b"last-order plane" in last_error(peel(desc(ALPHA), l=None))
    assert b"depth attachment" in last_error(peel(desc(ALPHA), z=None))
    # every legal mode and flag, and the kernels of one layer by name
    names = ctx.launches_of(lambda: (lib.sailor_hip_surface_peel_begin(ctx.handle, W, H, C.byref(band), ws, n, last.data_ptr(), 1),
                                     peel(desc(CULL | CUT | ALPHA))(), peel(desc(GLTF | CUT | (1 << SHIFT), prim_base=4), entry=gl, index=1)(),
                                     lib.sailor_hip_surface_peel_commit(ctx.handle, W, H, C.byref(band), ws, n, last.data_ptr(), count.data_ptr()),
                                     lib.sailor_hip_surface_blend(ctx.handle, plane.data_ptr(), plane.data_ptr(), None, ws, n, plane.data_ptr(), W, H, C.byref(band))))
    assert names == ["k_surface_begin", "k_surface_peel", "k_surface_peel_gltf", "k_surface_peel_commit", "k_surface_blend"], names
    ctx.synchronize()


# ---- timing -----------------------------------------------------------------------------------------------------------------------------------------------
def _grid_mesh(W, H, n):
    """n x n cells over the frame (and a little beyond), two triangles each, at distance 1 from the eye: scaled about the eye by an instance's model"""
    xs, ys = np.linspace(-1.05, 1.05, n + 1), np.linspace(-1.05, 1.05, n + 1)
    v = [cases.vertex((cases.EYE[0] + x * W / H, cases.EYE[1] + y, cases.EYE[2] - 1.0), (x, y)) for y in ys for x in xs]
    at = lambda i, j: j * (n + 1) + i
    t = [tri for j in range(n) for i in range(n) for tri in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))]
    return np.asarray(v, np.float32), np.asarray(t, np.uint32)


def test_launch_times_at_4k(ctx):
    """prints, at 3840 x 2160, for one and for four full-screen layers of 2 triangles and of 100 352 small triangles (an instance a layer), the medians of 5 of
    the peel draws, the commit and the blend of a layer and of the whole recorded pass with the real shade (six point lights).  No assertion on a value: the
    pass has no parent to compare against."""
    W, H = 3840, 2160
    cam_s = cases.deep_5(W, H)
    cam, lights = cam_s["cam"], cam_s["lights"]
    depth = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
    d_lights = upload_lights(lights, ctx.device)
    fp = ForwardPlus(ctx, W, H, len(lights))
    fp.cull(cam.frame, d_lights, len(lights), linearize_depth(ctx, cam.frame, depth))
    shade = lambda surface, ao: fp.shade(cam.frame, surface, d_lights, len(lights))
    target = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    meshes = {"2 triangles": (np.asarray(cases.wall(W, H, 1.0)[0], np.float32), np.asarray(cases.wall(W, H, 1.0)[1], np.uint32)), "100 352 triangles": _grid_mesh(W, H, 224)}
    for label, (v, t) in meshes.items():
        for layers in (1, 4):
            models = [host.transform_matrix([0.0, 150.0 * (1.0 - d), 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [d, d, d, 1.0]) for d in (50.0, 40.0, 80.0, 60.0)[:layers]]
            s = cases.cam_scene(W, H, [cases.blended(cases.draw(v, t), "alpha")], models=models, mats=cases.MATS, inst_materials=[0, 1, 2, 0][:layers])
            up = Uploaded(ctx, s)
            draws = [dict(d, blend="alpha") for d in up.draws]
            sp = SurfacePass(ctx, W, H)
            times = {"peel draw": [], "commit": [], "resolve": [], "blend": [], "whole pass": []}
            # the launches of one layer by name (begin, draw, commit, resolve, the shade's, blend), then the overflow round's three
            names = ctx.launches_of(lambda: sp.transparent(cam.frame, draws, up.instances, up.materials, up.textures, up.num_textures, depth, shade, target, layers=1))
            per_layer = len(names) - 3
            assert names[per_layer:] == ["k_surface_begin", "k_surface_peel", "k_surface_peel_commit"] and names[per_layer - 1] == "k_surface_blend", names
            slots = [(names.index(kernel), key) for kernel, key in (("k_surface_peel", "peel draw"), ("k_surface_peel_commit", "commit"), ("k_surface_resolve", "resolve"),
                                                                     ("k_surface_blend", "blend"))]
            for it in range(7):
                ctx.time_launches(0, per_layer * layers + 3)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                counts = sp.transparent(cam.frame, draws, up.instances, up.materials, up.textures, up.num_textures, depth, shade, target, layers=layers)
                stop.record()
                ctx.synchronize()
                if it >= 2:
                    times["whole pass"].append(start.elapsed_time(stop))
                    for k in range(layers):
                        for slot, key in slots:
                            times[key].append(ctx.timed_launch_ms(per_layer * k + slot))
            assert counts.cpu().numpy().tolist() == [W * H] * layers + [0]
            for key, x in times.items():
                print(f"[{label}, {layers} layer(s)] {key} 3840x2160: median {np.median(x) * 1e3:.1f} us (min {min(x) * 1e3:.1f}, max {max(x) * 1e3:.1f}, n={len(x)})")
            assert len(times["whole pass"]) == 5
            del up, sp
