"""The bucket route of the Transparent queue (sailor_amd/csrc/surface_buckets.hip) on the device, through the C-ABI and SurfacePass.transparent(mode="buckets"),
bit for bit throughout: (a) the planes after the draws and every layer read out of them against tests/transparent_ref.py on every case of
tests/transparent_cases.py; (b) Main and the counters against the peel route through the real shade; (c) two scenes of contention at budgets below, at and
above their depth, built three times; (d) a budget below the depth under a cutout; (e) orders at the top of the range; (f) two bands; (g) the recorded form in a
graph; (h) the refusals, which leave the store and the workspace untouched.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import transparent_cases as cases
import transparent_ref as tr
from sailor_amd import _lib, host
from sailor_amd.forward_plus import ForwardPlus, HipContext, SurfacePass, linearize_depth, upload_lights
from test_gltf_gpu import Uploaded
from test_surface_gpu import dev
from test_transparent_gpu import albedo_as_radiance, albedo_np, same

pytestmark = pytest.mark.gpu
EMPTY = np.uint64(2 ** 64 - 1)
W, H = 48, 32


# ---- the scenes of contention -----------------------------------------------------------------------------------------------------------------------------
def stack_40():
    """40 instances of one full-frame wall at 40 distinct distances (30 .. 69, not in drawing order), all in front of the depth attachment: 40 fragments a pixel
    from two large triangles an instance, the whole wave on one triangle at a time"""
    q = cases.wall(W, H, 1.0)
    distances = [30.0 + (7 * k) % 40 for k in range(40)]
    models = [host.transform_matrix([0.0, 150.0 * (1.0 - d), 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [d, d, d, 1.0]) for d in distances]
    return cases.cam_scene(W, H, [cases.blended(cases.draw(q[0], q[1]), "alpha")], models=models, mats=cases.MATS, inst_materials=[k % 3 for k in range(40)])


def grid_stack():
    """a 12 x 8 grid of 4 x 4-pixel quads x 16 coincident instances: 3072 small triangles, a lane each, so the 16 fragments of a pixel come from lanes of
    different waves (an instance is 192 lanes further on)"""
    v, t = [], []
    for j in range(8):
        for i in range(12):
            q = cases.wall(W, H, 50.0, -1 + 2 * i / 12, -1 + 2 * j / 8, -1 + 2 * (i + 1) / 12, -1 + 2 * (j + 1) / 8)
            t += [(len(v) + a, len(v) + b, len(v) + c) for a, b, c in q[1]]
            v += q[0]
    return cases.cam_scene(W, H, [cases.blended(cases.draw(v, t), "additive")], models=[cases.IDENTITY] * 16, mats=cases.MATS, inst_materials=[k % 3 for k in range(16)])


def big_orders_top():
    """order_abc with the largest primBase its 12 orders allow: orderPlus1 up to 2^32 - 3, a step below what EMPTY's high word would be"""
    s = cases.order_abc()
    s["prim_base"] = 2 ** 32 - 14
    return s


CONTENTION = {"stack_40": (stack_40, 40), "grid_stack": (grid_stack, 16)}


@pytest.fixture(scope="module")
def scenes():
    out = cases.all_scenes()
    out.update({name: build() for name, (build, _) in CONTENTION.items()})
    out["big_orders_top"] = big_orders_top()
    return out


@pytest.fixture(scope="module")
def restated(scenes):
    """name -> (depth attachment, layers, the fragments of every pixel): computed once, shared, left unchanged"""
    out = {}
    for name, s in scenes.items():
        depth = cases.depth_attachment(s)
        L, stats = tr.layers(s, depth)
        out[name] = (depth, L, stats["per_pixel"])
    for name, (_, deep) in CONTENTION.items():
        assert (out[name][2] == deep).all(), name
    return out


def planes_of(L, K, rows=slice(None)):
    """the reference's layers re-keyed as the store holds them: plane p = orderPlus1 << 32 | zbits of layer p, EMPTY where the pixel has no such fragment"""
    shape = L[0]["last"][rows].shape
    out = np.full((K + 1,) + shape, EMPTY, np.uint64)
    for p in range(min(K + 1, len(L))):
        c = L[p]["covered"][rows]
        key = (L[p]["last"][rows].astype(np.uint64) << np.uint64(32)) | np.ascontiguousarray(L[p]["z"][rows]).view(np.uint32).astype(np.uint64)
        out[p][c] = key[c]
    return out


def run(ctx, s, depth, shade, target, layers, band=None, up=None, on_layer=None, mode="buckets"):
    """the scene through SurfacePass.transparent -> (the band's rows of the target, the counters, the pass)"""
    up = up or Uploaded(ctx, s)
    draws = [dict(d, blend=sd["blend"]) for d, sd in zip(up.draws, s["draws"])]
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=len(draws))
    rows = slice(sp.band.fbRowBegin, sp.band.fbRowBegin + sp.band.fbRowCount)
    t = dev(ctx, target[rows])
    counts = sp.transparent(s["cam"].frame, draws, up.instances, up.materials, up.textures, up.num_textures, dev(ctx, depth), shade, t, layers=layers,
                            prim_base=s.get("prim_base", 0), on_layer=None if on_layer is None else (lambda *a: on_layer(sp, *a)), mode=mode)
    ctx.synchronize()
    return t.cpu().numpy(), counts.cpu().numpy(), sp


# ---- (a) the planes and every layer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.CASES))
def test_the_planes_and_every_layer_of_every_case_against_the_restatement(ctx, scenes, restated, name):
    s = scenes[name]
    depth, L, per_pixel = restated[name]
    K = len(L)
    seen = []

    def on_layer(sp, k, surface, cov, emissive, ao):
        ctx.synchronize()
        seen.append(dict(planes=surface.cpu().numpy(), covered=cov.cpu().numpy().astype(bool), emissive=None if emissive is None else emissive.cpu().numpy(),
                         ao=None if ao is None else ao.cpu().numpy(), keys=sp.download_keys()))
    got, counts, sp = run(ctx, s, depth, albedo_as_radiance, cases.target_of(s), K, on_layer=on_layer)
    planes = sp.download_buckets()
    np.testing.assert_array_equal(planes, planes_of(L, K), err_msg=f"{name}: the planes after the draws")
    assert (planes[K] == EMPTY).all() and (planes[0] != EMPTY).sum() == int((per_pixel > 0).sum())
    assert len(seen) == K and counts.tolist() == [int(l["covered"].sum()) for l in L] + [0], (counts.tolist(), K)
    for k, (g, want) in enumerate(zip(seen, L)):
        np.testing.assert_array_equal(g["covered"], want["covered"], err_msg=f"{name} layer {k}: coverage")
        np.testing.assert_array_equal(g["keys"], (want["z"].view(np.uint32).astype(np.uint64) << np.uint64(32)) | want["last"], err_msg=f"{name} layer {k}: keys")
        assert same(g["planes"], want["planes"]), f"{name} layer {k}: planes"
        if g["emissive"] is not None:
            assert same(g["emissive"], want["emissive"]) and same(g["ao"], want["ao_out"]), f"{name} layer {k}: emissive / aoOut"
        else:
            assert (want["emissive"] == tr.gltf_ref.NO_EMISSIVE).all()
    assert same(got, tr.composite(L, albedo_np, cases.target_of(s)))


# ---- (b) the two routes -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["order_abc", "mixed_modes", "cutout_gltf", "hostile_alpha"])
def test_main_and_the_counters_equal_the_peel_routes_through_the_real_shade(ctx, scenes, restated, name):
    s = scenes[name]
    depth, L, _ = restated[name]
    lights, cam = s["lights"], s["cam"]
    fp = ForwardPlus(ctx, s["W"], s["H"], len(lights))
    d_lights = upload_lights(lights, ctx.device)
    fp.cull(cam.frame, d_lights, len(lights), linearize_depth(ctx, cam.frame, dev(ctx, depth)))
    shade = lambda surface, ao: fp.shade(cam.frame, surface, d_lights, len(lights))
    tgt, up = cases.target_of(s), Uploaded(ctx, s)
    for layers in (len(L), 2):    # the whole depth, and a budget below it: an overflow on both routes
        peel, peel_counts, _ = run(ctx, s, depth, shade, tgt, layers, up=up, mode="peel")
        buckets, bucket_counts, _ = run(ctx, s, depth, shade, tgt, layers, up=up, mode="buckets")
        np.testing.assert_array_equal(buckets.view(np.uint32), peel.view(np.uint32), err_msg=f"{name}, {layers} layers: Main")
        assert bucket_counts.tolist() == peel_counts.tolist() and (layers == len(L)) == (peel_counts[layers] == 0), (peel_counts, bucket_counts)
        assert (peel.view(np.uint32) != tgt.view(np.uint32)).any(axis=-1).sum() > 100, "the pass blends"


# ---- (c) contention -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 8, 39, 40, 64])
@pytest.mark.parametrize("name", list(CONTENTION))
def test_contended_pixels_keep_their_first_k_orders_whatever_the_schedule(ctx, scenes, restated, name, K):
    s = scenes[name]
    depth, L, per_pixel = restated[name]
    want = planes_of(L, K)
    up, tgt = Uploaded(ctx, s), cases.target_of(s)
    for build in range(3):
        _, counts, sp = run(ctx, s, depth, albedo_as_radiance, tgt, K, up=up)
        planes = sp.download_buckets()
        np.testing.assert_array_equal(planes, want, err_msg=f"{name}, K = {K}, build {build}")
        assert counts[K] == int((per_pixel > K).sum()) and counts[:K].tolist() == [int((per_pixel > k).sum()) for k in range(K)], (name, K, counts)
    deep = CONTENTION[name][1]
    assert (planes[min(K, deep - 1)] != EMPTY).all() and (K < deep) == (counts[K] == W * H) and (K < deep or counts[K] == 0)


# ---- (d) a budget below the depth under a cutout ------------------------------------------------------------------------------------------------------------
def test_a_discarded_fragment_occupies_no_plane_at_a_budget_of_one(ctx, scenes, restated):
    """cutout_gltf at K = 1: where the second draw's fragment is discarded the sentinel holds the THIRD draw's, or nothing -- a discarded fragment that reached
    a slot would show as a foreign key or as an overflow that is not there"""
    s = scenes["cutout_gltf"]
    depth, L, per_pixel = restated["cutout_gltf"]
    discarded_everywhere = tr.layers(s, depth, discarded_take_a_layer=True)[0]
    want, mutant = planes_of(L, 1), planes_of(discarded_everywhere, 1)
    assert (want != mutant).sum() > 20, "the case separates the two"
    got, counts, sp = run(ctx, s, depth, albedo_as_radiance, cases.target_of(s), 1)
    np.testing.assert_array_equal(sp.download_buckets(), want)
    assert counts.tolist() == [int(L[0]["covered"].sum()), int((per_pixel > 1).sum())]
    assert same(got, tr.composite(L, albedo_np, cases.target_of(s), limit=1))


# ---- (e) the top of the order range -------------------------------------------------------------------------------------------------------------------------
def test_orders_near_the_top_of_the_range_sort_as_unsigned(ctx, scenes, restated):
    """big_orders (in (a): its orders straddle 2^31, the sign bit of the key's high word) and the same scene at the largest primBase: orderPlus1 up to 2^32 - 3"""
    s = scenes["big_orders_top"]
    depth, L, _ = restated["big_orders_top"]
    _, counts, sp = run(ctx, s, depth, albedo_as_radiance, cases.target_of(s), 3)
    planes = sp.download_buckets()
    np.testing.assert_array_equal(planes, planes_of(L, 3))
    taken = planes[:3][planes[:3] != EMPTY] >> np.uint64(32)
    assert taken.min() == 2 ** 32 - 13 and taken.max() == 2 ** 32 - 3 and counts.tolist() == [int(l["covered"].sum()) for l in L] + [0]
    three = planes[2] != EMPTY
    assert three.sum() > 30 and (planes[0][three] < planes[1][three]).all() and (planes[1][three] < planes[2][three]).all()


# ---- (f) bands ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["order_abc", "cutout_gltf", "near_cut"])
def test_two_bands_give_the_whole_frames_bits(ctx, scenes, restated, name):
    s = scenes[name]
    depth, L, _ = restated[name]
    K = len(L) - 1   # a budget below the depth: the sentinel plane is in use
    tgt, up = cases.target_of(s), Uploaded(ctx, s)
    whole, counts, sp = run(ctx, s, depth, albedo_as_radiance, tgt, K, up=up)
    whole_planes = sp.download_buckets()
    np.testing.assert_array_equal(whole_planes, planes_of(L, K))
    parts, planes, totals = [], [], 0
    for rank in reversed(range(2)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
        band = host.band_for_rank(s["W"], s["H"], rank, 2)
        got, c, p = run(ctx, s, depth, albedo_as_radiance, tgt, K, band=band, up=up)
        assert 0 < band.fbRowCount < s["H"]
        parts.append(got)
        planes.append(p.download_buckets())
        totals += c.astype(np.int64)
    np.testing.assert_array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    np.testing.assert_array_equal(np.concatenate(planes, axis=1), whole_planes)
    assert totals.tolist() == counts.tolist() and counts[K] > 0


# ---- (g) the recorded form in a graph -----------------------------------------------------------------------------------------------------------------------
def test_the_recorded_form_captured_into_a_graph_and_replayed(ctx, scenes, restated):
    s = scenes["mixed_modes"]
    depth, L, _ = restated["mixed_modes"]
    tgt = cases.target_of(s)
    eager, eager_counts, _ = run(ctx, s, depth, albedo_as_radiance, tgt, 2)
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
            out.copy_(sp.transparent(s["cam"].frame, draws, up.instances, up.materials, up.textures, up.num_textures, d_depth, albedo_as_radiance, work, layers=2,
                                     mode="buckets"))
        for _ in range(2):
            work.fill_(7.0)       # a fresh target, stale counters and a store full of foreign keys: the replay owes nothing to what it finds
            out.zero_()
            sp.buckets.fill_(12345)
            graph.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(work.cpu().numpy().view(np.uint32), eager.view(np.uint32))
            assert out.cpu().numpy().tolist() == eager_counts.tolist()
            np.testing.assert_array_equal(sp.download_buckets(), planes_of(L, 2))
    finally:
        c2.close()


# ---- (h) refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_say_why_and_leave_the_store_and_the_workspace_untouched(ctx, scenes):
    lib = ctx._lib
    s = scenes["cutout_gltf"]
    Wc, Hc = s["W"], s["H"]
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, Wc, Hc, max_draws=2)
    ws, n, band, frame = sp.workspace.data_ptr(), sp.workspace.numel(), sp.band, s["cam"].frame
    bad_band = _lib.Band(0, 1, 3, 16)
    K = 4
    nb = lib.sailor_hip_surface_bucket_bytes(Wc, C.byref(band), K)
    assert nb == (K + 1) * Wc * Hc * 8
    store = torch.empty(nb // 8, dtype=torch.int64, device=ctx.device)
    depth = torch.zeros((Hc, Wc), dtype=torch.float32, device=ctx.device)
    count = torch.zeros(2, dtype=torch.int32, device=ctx.device)
    CUT, GLTF, CULL, SHIFT = _lib.SURFACE_ALPHA_CUTOUT, _lib.SURFACE_GLTF, _lib.SURFACE_CULL_BACK, _lib.SURFACE_BLEND_SHIFT
    ALPHA, MULTIPLY = _lib.SURFACE_BLEND_ALPHA << SHIFT, _lib.SURFACE_BLEND_MULTIPLY << SHIFT
    d = up.draws[1]

    def desc(flags, prim_base=0, vertices=d["vertices"].data_ptr()):
        return _lib.SurfaceDraw(vertices, d["indices"].data_ptr(), d["instance_ids"].data_ptr(), 2, 1, prim_base, flags, 0, 0)

    def draw(dd, entry=lib.sailor_hip_surface_bucket_draw, index=0, workspace=ws, size=n, b=band, mats=up.materials.data_ptr(), z=depth.data_ptr(), st=store.data_ptr(),
             sn=nb, layers=K):
        return lambda: entry(ctx.handle, C.byref(frame), C.byref(dd), up.instances.data_ptr(), mats, 3, up.textures.data_ptr(), up.num_textures, index, Wc, Hc, C.byref(b),
                             workspace, size, z, st, sn, layers)

    def begin(b=band, workspace=ws, size=n, st=store.data_ptr(), sn=nb, layers=K):
        return lambda: lib.sailor_hip_surface_bucket_begin(ctx.handle, Wc, Hc, C.byref(b), workspace, size, st, sn, layers)

    def layer(b=band, workspace=ws, size=n, st=store.data_ptr(), sn=nb, layers=K, k=0, c=count.data_ptr()):
        return lambda: lib.sailor_hip_surface_bucket_layer(ctx.handle, Wc, Hc, C.byref(b), workspace, size, st, sn, layers, k, c)
    gl = lib.sailor_hip_surface_bucket_draw_gltf
    invalid = {
        "bucket_begin: invalid band": begin(b=bad_band), "bucket_begin: null workspace": begin(workspace=None), "bucket_begin: workspace too small": begin(size=1000),
        "bucket_begin: null store": begin(st=None), "bucket_begin: misaligned store": begin(st=store.data_ptr() + 4), "bucket_begin: store too small": begin(sn=nb - 1),
        "bucket_begin: store too small for the layers": begin(layers=K + 1), "bucket_begin: 0 layers": begin(layers=0), "bucket_begin: 65 layers": begin(sn=2 ** 40, layers=65),
        "bucket_draw: unknown flag bits": draw(desc(ALPHA | 32)), "bucket_draw: the glTF flag": draw(desc(ALPHA | GLTF)),
        "bucket_draw: cutout without materials": draw(desc(ALPHA | CUT), mats=None), "bucket_draw: null depth": draw(desc(ALPHA), z=None),
        "bucket_draw: misaligned depth": draw(desc(ALPHA), z=depth.data_ptr() + 2), "bucket_draw: null store": draw(desc(ALPHA), st=None),
        "bucket_draw: misaligned store": draw(desc(ALPHA), st=store.data_ptr() + 4), "bucket_draw: store too small": draw(desc(ALPHA), sn=nb - 8),
        "bucket_draw: 0 layers": draw(desc(ALPHA), layers=0), "bucket_draw: 65 layers": draw(desc(ALPHA), sn=2 ** 40, layers=65),
        "bucket_draw: null vertices": draw(desc(ALPHA, vertices=None)), "bucket_draw: drawIndex >= maxDraws": draw(desc(ALPHA), index=2),
        "bucket_draw: primBase overflow": draw(desc(ALPHA, prim_base=2 ** 32 - 1 - 4)), "bucket_draw: invalid band": draw(desc(ALPHA), b=bad_band),
        "bucket_draw: workspace too small": draw(desc(ALPHA), size=1000),
        "bucket_draw_gltf: without the glTF flag": draw(desc(ALPHA | CUT), entry=gl), "bucket_draw_gltf: unknown flag bits": draw(desc(GLTF | ALPHA | 64), entry=gl),
        "bucket_draw_gltf: null store": draw(desc(GLTF | ALPHA), entry=gl, st=None), "bucket_draw_gltf: 65 layers": draw(desc(GLTF | ALPHA), entry=gl, sn=2 ** 40, layers=65),
        "bucket_layer: invalid band": layer(b=bad_band), "bucket_layer: null workspace": layer(workspace=None), "bucket_layer: workspace too small": layer(size=1000),
        "bucket_layer: null store": layer(st=None), "bucket_layer: misaligned store": layer(st=store.data_ptr() + 4), "bucket_layer: store too small": layer(sn=nb - 1),
        "bucket_layer: 0 layers": layer(layers=0), "bucket_layer: 65 layers": layer(sn=2 ** 40, layers=65), "bucket_layer: k > layers": layer(k=K + 1),
        "bucket_layer: null counter": layer(c=None), "bucket_layer: misaligned counter": layer(k=K, c=count.data_ptr() + 2),
    }
    unsupported = {"bucket_draw: Multiply": draw(desc(MULTIPLY)), "bucket_draw_gltf: Multiply": draw(desc(GLTF | MULTIPLY | CUT), entry=gl)}
    # a store and a workspace of known bytes: a refused call changes neither (bucket_begin's fill is not a kernel: the launch log alone would not see it)
    store.copy_(torch.arange(store.numel(), dtype=torch.int64, device=ctx.device))
    sp.workspace.copy_((torch.arange(n, device=ctx.device) % 251).to(torch.uint8))
    count.fill_(77)
    ctx.synchronize()
    before_store, before_ws = store.cpu().numpy().copy(), sp.workspace.cpu().numpy().copy()
    for status, calls in ((-1, invalid), (-7, unsupported)):
        for what, call in calls.items():
            before, _ = ctx.launch_log(0)
            assert call() == status, what
            after, _ = ctx.launch_log(0)
            assert after == before, f"{what}: launched {after - before} kernels"
            assert b"sailor_hip_surface_bucket_" in lib.sailor_hip_context_last_error(ctx.handle), what
    ctx.synchronize()
    np.testing.assert_array_equal(store.cpu().numpy(), before_store)
    np.testing.assert_array_equal(sp.workspace.cpu().numpy(), before_ws)
    assert count.cpu().numpy().tolist() == [77, 77]
    last_error = lambda call: (call(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"bucket_draw: unknown flags" in last_error(draw(desc(ALPHA | 32))) and b"Multiply" in last_error(draw(desc(MULTIPLY)))
    assert b"bucket store is NULL" in last_error(draw(desc(ALPHA), st=None)) and b"depth attachment" in last_error(draw(desc(ALPHA), z=None))
    assert b"layers is outside 1 .. 64" in last_error(begin(layers=0)) and b"k is beyond layers" in last_error(layer(k=K + 1))
    assert b"smaller than sailor_hip_surface_bucket_bytes" in last_error(layer(sn=nb - 1)) and b"counter" in last_error(layer(c=None))
    # every legal mode and flag, and the kernels of a pass by name; the sentinel's read-out leaves the workspace's keys alone
    count.zero_()
    names = ctx.launches_of(lambda: (begin()(), draw(desc(ALPHA))(), draw(desc(GLTF | CUT | CULL | (1 << SHIFT), prim_base=4), entry=gl, index=1)(), layer(k=0)()))
    assert names == ["k_surface_begin", "k_surface_bucket", "k_surface_bucket_gltf", "k_surface_bucket_layer"], names
    keys = sp.download_keys()
    assert ctx.launches_of(lambda: layer(k=K, c=count.data_ptr() + 4)()) == ["k_surface_bucket_layer"]
    np.testing.assert_array_equal(sp.download_keys(), keys)
    planes = store.cpu().numpy().view(np.uint64).reshape(K + 1, Hc, Wc)
    assert count.cpu().numpy().tolist() == [int((planes[0] != EMPTY).sum()), 0] and (planes[2:] == EMPTY).all() and (keys != 0).sum() == count[0].item() > 0
