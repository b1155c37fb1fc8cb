"""The multisampled surface pass (sailor_amd/csrc/surface_msaa.hip) on the device, through the C-ABI and SurfacePass.multisampled, bit for bit throughout:
(a) the store, every layer's keys, the weights, the uncovered bytes, both counters and the accumulate of every case of tests/msaa_cases.py at 2, 4 and 8
samples against tests/msaa_ref.py, and at one sample against SurfacePass.draw's own keys; (b) through the real shade, interior pixels against the single-sample
pipeline's Main; (c) a contended fan under three schedules; (d) orders at the top of the range; (e) two bands; (f) a pass begun from its own sample depths, the
sample depths and the AVERAGE depth; (g) the recorded form in a graph over a store full of foreign keys; (h) the refusals, which leave store, workspace and
target untouched.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import msaa_cases as cases
import msaa_ref as mr
import surface_cases
import surface_ref
import transparent_cases
from sailor_amd import _lib, host
from sailor_amd.forward_plus import ForwardPlus, HipContext, SurfacePass, linearize_depth, upload_lights
from test_surface_gpu import Uploaded, dev
from test_transparent_gpu import albedo_as_radiance, same

pytestmark = pytest.mark.gpu
LOW = np.uint64(0xFFFFFFFF)
_scenes, _restated = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = cases.CASES[name]()
    return _scenes[name]


def restated(name, S, rows=None):
    """the restatement of a case at S samples: computed once, shared, left unchanged"""
    key = (name, S, rows)
    if key not in _restated:
        _restated[key] = mr.render(scene(name), host.msaa_sample_positions(S), rows=rows)
    return _restated[key]


def draws_of(up):
    return [dict(vertices=v, indices=i if len(d["indices"]) else i[:0], instance_ids=ids, num_drawn=d["num_drawn"], first_instance=d["first_instance"],
                 cull_back=d["cull_back"], alpha_cutout=d.get("alpha_cutout", False)) for v, i, ids, d in up.draws]


def run(ctx, s, S, target=None, layers=None, band=None, up=None, shade=albedo_as_radiance, sample_depth=None, frame=None):
    """the scene through SurfacePass.multisampled -> dict(main, counts, store, per layer: keys, radiance, weight; uncovered, sp)"""
    up = up or Uploaded(ctx, s)
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=max(len(s["draws"]), 1))
    rows = slice(sp.band.fbRowBegin, sp.band.fbRowBegin + sp.band.fbRowCount)
    t = dev(ctx, (cases.constant_target(s) if target is None else target)[rows])
    seen = []

    def on_layer(k, surface, weight, emissive, ao):
        ctx.synchronize()
        seen.append(dict(keys=sp.download_keys(), radiance=shade(surface, ao).cpu().numpy(), weight=weight.cpu().numpy().copy()))
    counts = sp.multisampled(frame or up.frame, draws_of(up), up.instances, up.materials, up.textures, up.num_textures, shade, t, samples=S, layers=layers,
                             sample_depth=None if sample_depth is None else dev(ctx, sample_depth), prim_base=s.get("prim_base", 0), on_layer=on_layer)
    ctx.synchronize()
    return dict(main=t.cpu().numpy(), counts=counts.cpu().numpy(), store=sp.download_samples(), seen=seen, uncovered=sp.uncovered.cpu().numpy(), sp=sp, up=up)


def single(ctx, s, up, shade=None, target=None, frame=None):
    """the single-sample pipeline over the same draws: begin, draw / draw_masked, resolve, the shade, composite -> (keys, Main | None, depth)"""
    sp = SurfacePass(ctx, s["W"], s["H"], max_draws=max(len(s["draws"]), 1))
    sp.begin(prim_base=s.get("prim_base", 0))
    for d in draws_of(up):
        sp.draw(frame or up.frame, instances=up.instances, materials=up.materials, textures=up.textures, num_textures=up.num_textures, **d)
    surface, depth, _ = sp.resolve(frame or up.frame, up.instances, up.materials, up.textures, up.num_textures)
    main = None if shade is None else sp.composite(shade(surface, None), dev(ctx, target)).cpu().numpy()
    return sp.download_keys(), main, depth


def accumulated(got, target, S):
    """rule 9 restated over the GPU's own per-layer radiance"""
    out = np.array(target, np.float32)
    for k, layer in enumerate(got["seen"]):
        out = mr.accumulate(out, layer["radiance"], layer["weight"], got["uncovered"], S, k)
    return out


def assert_layers(got, want_store, S, L, what):
    want = mr.layers(want_store, L)
    assert len(got["seen"]) == L, what
    for k, layer in enumerate(got["seen"]):
        np.testing.assert_array_equal(layer["keys"], want["keys"][k], err_msg=f"{what} layer {k}: keys")
        np.testing.assert_array_equal(layer["weight"], want["weights"][k], err_msg=f"{what} layer {k}: weights")
    np.testing.assert_array_equal(got["uncovered"], want["uncovered"], err_msg=f"{what}: uncovered")
    assert got["counts"].tolist() == [int(c) for c in want["counts"]] + [want["clipped"]], (what, got["counts"].tolist())
    return want


# ---- (a) every case -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_store_layers_weights_counters_and_accumulate_of_every_case_against_the_restatement(ctx, name, S):
    s = scene(name)
    want = restated(name, S)
    target = cases.constant_target(s)
    got = run(ctx, s, S, target)
    np.testing.assert_array_equal(got["store"], want["store"], err_msg=f"{name} x{S}: the store")
    assert_layers(got, want["store"], S, S, f"{name} x{S}")
    assert same(got["main"], accumulated(got, target, S)), f"{name} x{S}: Main"
    if S > 2:   # a budget below the sample count: clipped samples go to the last layer
        few = run(ctx, s, S, target, layers=2, up=got["up"])
        np.testing.assert_array_equal(few["store"], want["store"])
        folded = assert_layers(few, want["store"], S, 2, f"{name} x{S}, two layers")
        assert same(few["main"], accumulated(few, target, S))
        assert name != "eight_owners" or S != 8 or folded["clipped"] > 0
    if name == "high_orders":
        assert int((want["store"] & LOW).max()) == 2 ** 32 - 3 and int((got["store"] & LOW).max()) == 2 ** 32 - 3   # the top of the low word: sorts as unsigned


@pytest.mark.parametrize("name", list(cases.CASES))
def test_at_one_sample_the_store_is_the_single_sample_draws_keys(ctx, name):
    s = scene(name)
    up = Uploaded(ctx, s)
    got = run(ctx, s, 1, up=up)
    keys, _, _ = single(ctx, s, up)
    np.testing.assert_array_equal(got["store"][..., 0], keys, err_msg=name)
    np.testing.assert_array_equal(got["seen"][0]["keys"], np.where(keys & LOW != 0, keys, np.uint64(0)))
    assert set(np.unique(got["seen"][0]["weight"]).tolist()) <= {0, 1}


# ---- the glTF draw ----------------------------------------------------------------------------------------------------------------------------------------
GLTF_CASES = ("cutoff_exact", "cutoff_per_instance", "cutoff_tie_discarded", "large_cutout_two_superblocks", "mixed_pass", "normal_matrix_near_plane")


def run_gltf(ctx, s, S, up):
    """a scene of tests/gltf_cases.py through multisampled() (a draw that carries gltf goes through sailor_hip_surface_msaa_draw_gltf) -> the pass"""
    sp = SurfacePass(ctx, s["W"], s["H"], max_draws=max(len(s["draws"]), 1))
    t = dev(ctx, cases.constant_target(s))
    ao = None if up.ao_in is None else dev(ctx, up.ao_in)
    sp.multisampled(up.frame, up.draws, up.instances, up.materials, up.textures, up.num_textures, albedo_as_radiance, t, samples=S, ao_in=ao, prim_base=s.get("prim_base", 0))
    return sp


@pytest.mark.parametrize("name", GLTF_CASES)
def test_the_gltf_draw_at_one_sample_issues_the_keys_of_sailor_hip_surface_draw_gltf(ctx, name):
    """baseColorFactor's alpha against the material's alphaCutoff, per instance, at a tie, in a large triangle, mixed with Standard draws: at one sample the
    store is the single-sample glTF pass's keys"""
    import gltf_cases
    import test_gltf_gpu
    s = gltf_cases.CASES[name][0]()
    up = test_gltf_gpu.Uploaded(ctx, s)
    want = test_gltf_gpu.run(ctx, s, up=up)["keys"]
    launched = ctx.launches_of(lambda: run_gltf(ctx, s, 1, up))
    assert "k_surface_msaa_gltf" in launched and ("k_surface_msaa" in launched) == any(not d["gltf"] for d in up.draws), launched
    sp = run_gltf(ctx, s, 1, up)
    np.testing.assert_array_equal(sp.download_samples()[..., 0], want, err_msg=name)
    assert (want & LOW != 0).any()


def test_an_opaque_gltf_draw_at_eight_samples_issues_the_standard_draws_store(ctx):
    import gltf_cases
    import test_gltf_gpu
    for name in ("near_plane", "staircase", "triangle_larger_than_the_frame", "eight_owners"):
        s = gltf_cases.as_gltf(scene(name))
        sp = run_gltf(ctx, s, 8, test_gltf_gpu.Uploaded(ctx, s))
        np.testing.assert_array_equal(sp.download_samples(), restated(name, 8)["store"], err_msg=name)


# ---- (b) through the real shade -------------------------------------------------------------------------------------------------------------------------------
def shaded_scene(name):
    s = surface_cases.materials_and_normal_map() if name == "materials_and_normal_map" else surface_cases.boxes_and_ground(8, 64, 48)
    near = 1.0 if name == "materials_and_normal_map" else 0.5
    frame = host.fill_frame_data(np.eye(4, dtype=np.float32).reshape(16), 90.0, near, 20000.0, s["W"], s["H"])   # the scenes' camera: the eye at the origin, down -z
    frame.view[:] = [float(x) for x in s["view"]]
    frame.projection[:] = [float(x) for x in s["projection"]]
    lights = transparent_cases.lights()
    lights["worldPosition"][:, 1] -= np.float32(150.0)
    return s, frame, lights


@pytest.mark.parametrize("name", ["materials_and_normal_map", "boxes_and_ground"])
def test_interior_pixels_have_the_single_sample_pipelines_main_and_edge_pixels_the_restated_average(ctx, name):
    """Every pixel all of whose eight samples belong to the primitive that also wins the single-sample pass has the single-sample pipeline's Main bits; the
    others the restated average of the GPU's layer colours.  The interior share is taken over the pixels the pass owns a sample of, known from the restatement
    beforehand: 110 of 203 (0.54) on materials_and_normal_map and 1472 of 1554 (0.95) on boxes_and_ground(8, 64, 48).  (Of the whole FRAME they are 0.038 and
    0.479: the two scenes leave most, and just over half, of their frame to the sky, so no pass over them can own half the frame.)"""
    s, frame, lights = shaded_scene(name)
    S = 8
    want = mr.render(s, host.msaa_sample_positions(S))
    one = surface_ref.render(s)["keys"] & LOW
    orders = want["store"] & LOW
    interior = (orders == one[..., None]).all(-1) & (one != 0)
    edge = (orders != orders[..., :1]).any(-1)
    touched = (orders != 0).any(-1)
    print(f"{name}: of the frame {interior.mean():.3f} interior, {edge.mean():.3f} edge; of the {touched.sum()} pixels the pass owns a sample of, {interior.sum() / touched.sum():.3f} interior")
    assert interior.sum() / touched.sum() > 0.5 and edge.mean() > 0.0
    up = Uploaded(ctx, s)
    fp = ForwardPlus(ctx, s["W"], s["H"], len(lights))
    d_lights = upload_lights(lights, ctx.device)
    keys, _, depth = single(ctx, s, up, frame=frame)
    fp.cull(frame, d_lights, len(lights), linearize_depth(ctx, frame, depth))
    shade = lambda surface, ao: fp.shade(frame, surface, d_lights, len(lights))
    rng = np.random.default_rng(4)
    target = rng.uniform(0, 1, (s["H"], s["W"], 4)).astype(np.float32)
    _, main1, _ = single(ctx, s, up, shade, target, frame=frame)
    got = run(ctx, s, S, target, up=up, shade=shade, frame=frame)
    np.testing.assert_array_equal(got["store"], want["store"])
    np.testing.assert_array_equal(keys & LOW, one)
    np.testing.assert_array_equal(got["main"][interior].view(np.uint32), main1[interior].view(np.uint32), err_msg="interior pixels: the single-sample pipeline's bits")
    assert (main1[interior][:, :3] > 0.001).any() and (main1[interior].view(np.uint32) != target[interior].view(np.uint32)).any(), "the covered pixels are lit"
    assert same(got["main"], accumulated(got, target, S)), "edge pixels: the restated average of the layers' colours"
    nothing = (orders == 0).all(-1)
    np.testing.assert_array_equal(got["main"][nothing].view(np.uint32), target[nothing].view(np.uint32))
    assert (got["main"][edge].view(np.uint32) != main1[edge].view(np.uint32)).any(), "an edge pixel is an average, not the winner"


# ---- (c) contention ---------------------------------------------------------------------------------------------------------------------------------------
def fan_as_draws(reverse=False):
    """the fan a triangle a draw, two empty draws between them (eight draws; the orders are the one draw's), or the same in reversed order"""
    s = surface_cases.fan_around_a_pixel_centre()
    v, tris = s["draws"][0]["vertices"], [tuple(int(q) for q in t) for t in s["draws"][0]["indices"]]
    tris = tris[::-1] if reverse else tris
    empty = surface_cases.draw(v, np.zeros((0, 3), np.uint32))
    each = [surface_cases.draw(v, [t]) for t in tris]
    return dict(s, draws=each[:2] + [empty] + each[2:5] + [empty] + each[5:])


def test_the_fan_as_one_draw_as_eight_draws_and_reversed_gives_the_same_store_and_main(ctx):
    one, eight, back = surface_cases.fan_around_a_pixel_centre(), fan_as_draws(), fan_as_draws(reverse=True)
    P8 = host.msaa_sample_positions(8)
    want, want_back = mr.render(one, P8), mr.render(back, P8)
    np.testing.assert_array_equal(mr.render(eight, P8)["store"], want["store"])
    assert ((want["store"] & LOW != 0) == (want_back["store"] & LOW != 0)).all() and (want["store"] >> np.uint64(32) == want_back["store"] >> np.uint64(32)).all()
    mains = []
    for s, w in ((one, want), (eight, want), (back, want_back)):
        up = Uploaded(ctx, s)
        for build in range(3):
            got = run(ctx, s, 8, up=up)
            np.testing.assert_array_equal(got["store"], w["store"])
            mains.append(got["main"])
    for m in mains[1:]:   # one material, one colour: the average does not depend on which triangle owns which sample
        np.testing.assert_array_equal(m.view(np.uint32), mains[0].view(np.uint32))
    assert mr.layers(want["store"], 8)["counts"][1] > 0   # the fan's spokes: pixels with two owners


# ---- (e) two bands ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.BAND_CASES)
def test_two_bands_give_the_whole_frames_bits(ctx, name):
    s = scene(name)
    whole = restated(name, 8)
    target = cases.constant_target(s)
    up = Uploaded(ctx, s)
    full = run(ctx, s, 8, target, up=up)
    stores, mains = [], []
    for rank in reversed(range(2)):   # tile row 0 is the bottom of the framebuffer: the last rank's band holds the first rows
        band = host.band_for_rank(s["W"], s["H"], rank, 2)
        got = run(ctx, s, 8, target, band=band, up=up)
        np.testing.assert_array_equal(got["store"], mr.render(s, host.msaa_sample_positions(8), rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount))["store"])
        stores.append(got["store"]); mains.append(got["main"])
    np.testing.assert_array_equal(np.concatenate(stores), whole["store"])
    np.testing.assert_array_equal(np.concatenate(mains).view(np.uint32), full["main"].view(np.uint32))


# ---- (f) depth ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 8])
def test_sample_depths_the_average_depth_and_a_pass_begun_from_its_own_prepass(ctx, S):
    s = scene("prepass_scene")
    want = restated("prepass_scene", S)
    first = run(ctx, s, S)
    depth = torch.full((s["H"], s["W"]), 7.0, dtype=torch.float32, device=ctx.device)
    samples, _ = first["sp"].store_sample_depth(depth)
    ctx.synchronize()
    z, average = mr.depth_out(want["store"])
    np.testing.assert_array_equal(samples.cpu().numpy().view(np.uint32), z.view(np.uint32))
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), average.view(np.uint32))
    assert len(np.unique(z)) >= 4 and ((average > z.min(-1)) & (average < z.max(-1))).any()   # pixels whose samples lie at different depths
    again = run(ctx, s, S, sample_depth=samples.cpu().numpy(), up=first["up"])     # GreaterOrEqual: the same draws own the same samples at the same depth
    np.testing.assert_array_equal(again["store"], first["store"])
    np.testing.assert_array_equal(again["store"], mr.render(s, host.msaa_sample_positions(S), sample_depth=z)["store"])
    nearer = np.where(z > 0, np.float32(0.99), np.float32(0.0)).astype(np.float32)   # a prepass in front of everything: nothing of the pass is visible
    hidden = run(ctx, s, S, sample_depth=nearer, up=first["up"])
    assert not (hidden["store"] & LOW).any() and hidden["counts"].tolist() == [0] * (S + 1)
    np.testing.assert_array_equal(hidden["main"].view(np.uint32), cases.constant_target(s).view(np.uint32))


# ---- (g) the recorded form in a graph -----------------------------------------------------------------------------------------------------------------------
def test_the_recorded_form_captured_into_a_graph_and_replayed_over_foreign_keys(ctx):
    s = scene("eight_owners")
    target = cases.constant_target(s)
    eager = run(ctx, s, 8, target, layers=4)
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        up = Uploaded(c2, s)
        sp = SurfacePass(c2, s["W"], s["H"], max_draws=len(s["draws"]))
        seed, work = dev(ctx, target), dev(ctx, np.zeros_like(target))
        out = torch.zeros(5, dtype=torch.int32, device=ctx.device)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            work.copy_(seed)      # the pass rewrites its target in place: every replay starts from the seed
            out.copy_(sp.multisampled(up.frame, draws_of(up), up.instances, up.materials, up.textures, up.num_textures, albedo_as_radiance, work, samples=8, layers=4))
        for _ in range(2):
            work.fill_(7.0)
            out.zero_()
            sp.sample_store.fill_(-1)      # foreign keys: all ones, above every key of the pass
            sp.workspace.fill_(0xA5)
            graph.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(work.cpu().numpy().view(np.uint32), eager["main"].view(np.uint32))
            np.testing.assert_array_equal(sp.download_samples(), eager["store"])
            assert out.cpu().numpy().tolist() == eager["counts"].tolist() and out[4].item() > 0
    finally:
        c2.close()


# ---- (h) refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_store_workspace_and_target_untouched(ctx):
    lib = ctx._lib
    s = scene("cutout_at_the_edge")
    W, H, S = s["W"], s["H"], 8
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, W, H, max_draws=2)
    sp.workspace.fill_(0x5A)
    ws, n, band, frame = sp.workspace.data_ptr(), sp.workspace.numel(), sp.band, up.frame
    bad_band = _lib.Band(0, 1, 3, 16)
    nb = lib.sailor_hip_surface_msaa_bytes(W, C.byref(band), S)
    store = torch.full((nb // 8,), 0x1234567, dtype=torch.int64, device=ctx.device)
    plane = torch.full((H, W, 4), 3.0, dtype=torch.float32, device=ctx.device)
    bytes_ = torch.full((H, W), 9, dtype=torch.uint8, device=ctx.device)
    count = torch.zeros(2, dtype=torch.int32, device=ctx.device)
    before = [t.clone() for t in (sp.workspace, store, plane, bytes_, count)]
    CUT, GLTF, SHIFT = _lib.SURFACE_ALPHA_CUTOUT, _lib.SURFACE_GLTF, _lib.SURFACE_BLEND_SHIFT
    v, i, ids, d = up.draws[1]

    def desc(flags, prim_base=0, vertices=v.data_ptr()):
        return _lib.SurfaceDraw(vertices, i.data_ptr(), None, 2, 1, prim_base, flags, 0, 0)

    def draw(dd, entry=lib.sailor_hip_surface_msaa_draw, index=0, workspace=ws, size=n, b=band, mats=up.materials.data_ptr(), st=store.data_ptr(), sn=nb, samples=S):
        return lambda: entry(ctx.handle, C.byref(frame), C.byref(dd), up.instances.data_ptr(), mats, 1, up.textures.data_ptr(), up.num_textures, index, W, H, C.byref(b),
                             workspace, size, st, sn, samples)

    def layer(samples=S, layers=S, k=0, st=store.data_ptr(), sn=nb, weight=bytes_.data_ptr(), un=bytes_.data_ptr(), c=count.data_ptr(), cl=None, b=band):
        return lambda: lib.sailor_hip_surface_msaa_layer(ctx.handle, W, H, C.byref(b), ws, n, st, sn, samples, layers, k, weight, un, c, cl)

    def acc(samples=S, k=0, r=plane.data_ptr(), e=None, weight=bytes_.data_ptr(), un=bytes_.data_ptr(), t=plane.data_ptr(), b=band):
        return lambda: lib.sailor_hip_surface_msaa_accumulate(ctx.handle, r, e, weight, un, samples, k, t, W, H, C.byref(b))
    gl = lib.sailor_hip_surface_msaa_draw_gltf
    invalid = {
        "begin: three samples": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, store.data_ptr(), nb, 3, None),
        "begin: sixteen samples": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, store.data_ptr(), 2 * nb, 16, None),
        "begin: null store": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, None, nb, S, None),
        "begin: misaligned store": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, store.data_ptr() + 8, nb, S, None),
        "begin: small store": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, store.data_ptr(), nb - 8, S, None),
        "begin: misaligned sample depth": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, store.data_ptr(), nb, S, plane.data_ptr() + 2),
        "begin: invalid band": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(bad_band), ws, n, store.data_ptr(), nb, S, None),
        "begin: null workspace": lambda: lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), None, n, store.data_ptr(), nb, S, None),
        "draw: five samples": draw(desc(CUT), samples=5),
        "draw: null store": draw(desc(CUT), st=None),
        "draw: misaligned store": draw(desc(CUT), st=store.data_ptr() + 8),
        "draw: small store": draw(desc(CUT), sn=nb // 2),
        "draw: a blend mode": draw(desc(CUT | (2 << SHIFT))),
        "draw: the glTF flag": draw(desc(GLTF)),
        "draw: unknown flag bits": draw(desc(64)),
        "draw: cutout without materials": draw(desc(CUT), mats=None),
        "draw: null vertices": draw(desc(0, vertices=None)),
        "draw: drawIndex >= maxDraws": draw(desc(0), index=2),
        "draw: primBase overflow": draw(desc(0, prim_base=2 ** 32 - 1 - 4)),
        "draw: invalid band": draw(desc(0), b=bad_band),
        "draw: workspace too small": draw(desc(0), size=1000),
        "draw_gltf: without the glTF flag": draw(desc(CUT), entry=gl),
        "draw_gltf: a blend mode": draw(desc(GLTF | (1 << SHIFT)), entry=gl),
        "layer: six samples": layer(samples=6),
        "layer: no layers": layer(layers=0),
        "layer: more layers than samples": layer(layers=9),
        "layer: k at layers": layer(layers=4, k=4),
        "layer: null weight": layer(weight=None),
        "layer: layer 0 without uncovered": layer(un=None),
        "layer: null counter": layer(c=None),
        "layer: misaligned clipped counter": layer(cl=count.data_ptr() + 2),
        "layer: small store": layer(sn=nb - 1),
        "layer: invalid band": layer(b=bad_band),
        "accumulate: seven samples": acc(samples=7),
        "accumulate: k at samples": acc(k=8),
        "accumulate: null radiance": acc(r=None),
        "accumulate: null target": acc(t=None),
        "accumulate: misaligned emissive": acc(e=plane.data_ptr() + 4),
        "accumulate: null weight": acc(weight=None),
        "accumulate: layer 0 without uncovered": acc(un=None),
        "accumulate: invalid band": acc(b=bad_band),
        "store_depth: both outputs null": lambda: lib.sailor_hip_surface_msaa_store_depth(ctx.handle, store.data_ptr(), nb, S, None, None, W, H, C.byref(band)),
        "store_depth: misaligned depth": lambda: lib.sailor_hip_surface_msaa_store_depth(ctx.handle, store.data_ptr(), nb, S, None, plane.data_ptr() + 2, W, H, C.byref(band)),
        "store_depth: null store": lambda: lib.sailor_hip_surface_msaa_store_depth(ctx.handle, None, nb, S, plane.data_ptr(), None, W, H, C.byref(band)),
        "store_depth: nine samples": lambda: lib.sailor_hip_surface_msaa_store_depth(ctx.handle, store.data_ptr(), nb, 9, plane.data_ptr(), None, W, H, C.byref(band)),
    }
    for what, call in invalid.items():
        launched, _ = ctx.launch_log(0)
        assert call() == -1, what
        after, _ = ctx.launch_log(0)
        assert after == launched, f"{what}: launched {after - launched} kernels"
        assert b"sailor_hip_surface_msaa_" in lib.sailor_hip_context_last_error(ctx.handle), what
    ctx.synchronize()
    for t, was in zip((sp.workspace, store, plane, bytes_, count), before):
        assert torch.equal(t, was)
    last_error = lambda call: (call(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"msaa_draw: unknown flags" in last_error(draw(desc(CUT | (2 << SHIFT)))) and b"samples is not 1, 2, 4 or 8" in last_error(layer(samples=6))
    assert b"layers is outside 1 .. samples" in last_error(layer(layers=9)) and b"layer 0 needs the uncovered plane" in last_error(acc(un=None))
    # every legal flag, and the kernels of a pass of one layer by name
    names = ctx.launches_of(lambda: (lib.sailor_hip_surface_msaa_begin(ctx.handle, W, H, C.byref(band), ws, n, store.data_ptr(), nb, S, None),
                                     draw(desc(CUT | _lib.SURFACE_CULL_BACK))(), draw(desc(GLTF | CUT, prim_base=4), entry=gl, index=1)(),
                                     layer(layers=1, cl=count.data_ptr() + 4)(), acc()(),
                                     lib.sailor_hip_surface_msaa_store_depth(ctx.handle, store.data_ptr(), nb, S, None, plane.data_ptr(), W, H, C.byref(band))))
    assert names == ["k_surface_msaa_begin", "k_surface_begin", "k_surface_msaa", "k_surface_msaa_gltf", "k_surface_msaa_layer", "k_surface_msaa_accumulate",
                     "k_surface_msaa_store_depth"], names
    ctx.synchronize()
