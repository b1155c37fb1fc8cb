"""Row E4 as the reference runs it (GPU): RHISceneView::TraceScene through TOctree over the integer-truncated world boxes
(ECS/StaticMeshRendererECS.cpp:81,96,132; Containers/Octree.h:44-53,239-274), for the camera snapshot (sailor_hip_ecs_sweep_traced) and the cascade
mesh lists (sailor_hip_csm_caster_masks_traced), bit for bit against the literal octree of oracle.trace_scene_octree_boxes run on oracle.ecs_sweep's
world boxes.  Boxes whose truncation is undefined in C++ are held against the rule of include/sailor_hip.h instead (tests/trace_scene_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import trace_scene_cases as tc
from oracle import oracle
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import EcsSweep, csm_caster_masks

pytestmark = pytest.mark.gpu


def camera_planes(cam):
    planes, _ = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)
    return planes


def popcount(w: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(w).view(np.uint8)).sum())


def u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n, flips", [(1024, (0, 0)), (1 << 20, (75, 2))])
def test_octree_sweep_gives_the_references_visible_set(ctx, n, flips):
    """C1 and C5 under the 4K camera: octree-mode visibility and inserted words are the octree's; matrices and boxes are the flat mode's and the
    oracle's; against the flat sweep exactly the bits tests/test_oracle_cpu.py counts differ (75 seen only flat, 2 only through the octree at C5)."""
    ents = synth.make_entities(n)
    planes = camera_planes(synth.make_camera(3840, 2160))
    ow, oa, ov = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes)
    tv, ti, _, _ = oracle.trace_scene_octree_boxes(oa, planes)
    fw, fa, fv = EcsSweep(ctx, ents).run(planes)
    sw = EcsSweep(ctx, ents, trace="octree")
    w, a, v = sw.run(planes)
    ctx.synchronize()
    for got in (w, fw):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), ow.view(np.uint32))
    for got in (a, fa):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), oa.view(np.uint32))
    np.testing.assert_array_equal(u64(v), tv)
    np.testing.assert_array_equal(u64(sw.inserted), ti)
    assert popcount(ti) == n
    fv = u64(fv)
    np.testing.assert_array_equal(fv, ov)
    assert (popcount(fv & ~u64(v)), popcount(u64(v) & ~fv)) == flips


def test_octree_sweep_under_the_8k_camera(ctx):
    ents = synth.make_entities(1 << 20)
    planes = camera_planes(synth.make_camera(7680, 4320))
    _, oa, _ = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes)
    tv, ti, _, _ = oracle.trace_scene_octree_boxes(oa, planes)
    sw = EcsSweep(ctx, ents, trace="octree")
    _, a, v = sw.run(planes)
    ctx.synchronize()
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), oa.view(np.uint32))
    np.testing.assert_array_equal(u64(v), tv)
    np.testing.assert_array_equal(u64(sw.inserted), ti)


@pytest.mark.parametrize("root", [8192, 1000, 64])
def test_strict_root_containment_with_small_roots(ctx, root):
    """100 000 generated entities under roots too small for the scene: many are not inserted, and those are never visible"""
    ents = synth.make_entities(100000)
    planes = camera_planes(synth.make_camera(3840, 2160))
    _, oa, _ = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes)
    tv, ti, _, st = oracle.trace_scene_octree_boxes(oa, planes, root_size=root)
    sw = EcsSweep(ctx, ents, trace="octree", octree_root_size=root)
    _, _, v = sw.run(planes)
    ctx.synchronize()
    assert st["not_inserted"] > 10000
    np.testing.assert_array_equal(u64(v), tv)
    np.testing.assert_array_equal(u64(sw.inserted), ti)


def _caster_octree(ctx, aabb, planes, root):
    """sailor_hip_csm_caster_masks_traced on world boxes -> (masks [k, words], inserted [words], flat masks [k, words])"""
    d = torch.from_numpy(np.ascontiguousarray(aabb, np.float32)).to(ctx.device)
    ins = torch.full(((len(aabb) + 63) // 64,), -1, dtype=torch.int64, device=ctx.device)
    m = csm_caster_masks(ctx, d, planes, trace="octree", octree_root_size=root, inserted=ins)
    f = csm_caster_masks(ctx, d, planes)
    ctx.synchronize()
    return u64(m), u64(ins), u64(f)


def _sweep_octree(ctx, aabb, planes, root):
    """the same boxes as local boxes of root entities with identity TRS through sailor_hip_ecs_sweep_traced -> (world boxes, visibility, inserted)"""
    ents = tc.identity_entities(aabb)
    sw = EcsSweep(ctx, ents, trace="octree", octree_root_size=root)
    _, a, v = sw.run(planes)
    ctx.synchronize()
    _, oa, _ = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes)
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), oa.view(np.uint32))
    return oa, u64(v), u64(sw.inserted)


@pytest.mark.parametrize("case", ["truncation", "large", "faces64", "faces1000"])
def test_truncation_and_containment_edges(ctx, case):
    """hand-built world boxes (tests/trace_scene_cases.py): negative fractional centres, extents below one, finite inverted boxes, boxes the float and
    the integer test disagree on in both directions, centres above 2^24 under a root of 2^30, integer faces on +-h and one unit inside -- through the
    caster entry point (world boxes as given) and through the sweep (identity TRS)"""
    if case == "truncation":
        aabb, planes, root = tc.truncation_case()
    elif case == "large":
        aabb, planes, root = tc.large_case()
    else:
        aabb, root = tc.root_faces_case(int(case[5:]))
        planes = np.stack([tc.one_plane((0, 0, 0), 1.0), tc.camera_planes()])
    n = len(aabb)
    masks, ins, flat = _caster_octree(ctx, aabb, planes, root)
    exact = tc.walk_exact(aabb)
    disagree, hidden = [0, 0], 0
    for k in range(len(planes)):
        tv, ti, _, _ = oracle.trace_scene_octree_boxes(aabb, planes[k], root_size=root)
        rv, ri, _ = tc.trace_rule(aabb, planes[k], root)
        got, got_ins = tc.bits(masks[k], n), tc.bits(ins, n)
        np.testing.assert_array_equal(got, rv)                 # the documented rule, negative extents included
        np.testing.assert_array_equal(got_ins, ri)
        hidden += tc.check_against_the_walk(got, got_ins, tc.bits(tv, n), tc.bits(ti, n), aabb)
        np.testing.assert_array_equal(flat[k], oracle.csm_caster_masks(aabb, planes[k:k + 1])[0])
        fl, ref = tc.bits(flat[k], n), tc.bits(tv, n)
        disagree[0] += int((fl & ~ref)[exact].sum()); disagree[1] += int((ref & ~fl)[exact].sum())
        oa, v, si = _sweep_octree(ctx, aabb, planes[k], root)
        assert not tc.negative_extent(oa).any()                # AABB::Apply never yields min > max: the sweep's boxes are all exact
        sv, sins, _, _ = oracle.trace_scene_octree_boxes(oa, planes[k], root_size=root)
        np.testing.assert_array_equal(v, sv)
        np.testing.assert_array_equal(si, sins)
    if case == "truncation":
        assert disagree[0] > 0 and disagree[1] > 0 and hidden > 0
    if case.startswith("faces"):
        assert 0 < popcount(ins) < n


def test_undefined_boxes_are_neither_inserted_nor_visible(ctx):
    """NaN, +-Inf and +-3e9 centres or extents: not inserted, not visible, on both entry points; every other entity -- those sharing a word with them
    included -- is the oracle's, run with the undefined boxes moved outside the root (its C integer arithmetic would overflow on them)"""
    aabb, planes, root = tc.truncation_case()
    mixed = tc.with_undefined(aabb, every=7)          # several in one 64-entity word
    n = len(mixed)
    _, _, defined = tc.trace_rule(mixed, planes[3], root)
    assert (~defined).sum() == len(tc.UNDEFINED)
    masks, ins, _ = _caster_octree(ctx, mixed, planes, root)
    got_ins = tc.bits(ins, n)
    for k in range(len(planes)):
        tv, ti, _, _ = oracle.trace_scene_octree_boxes(tc.oracle_safe(mixed, defined, root), planes[k])
        got = tc.bits(masks[k], n)
        assert not got[~defined].any()
        np.testing.assert_array_equal(got, tc.trace_rule(mixed, planes[k], root)[0])
        tc.check_against_the_walk(got, got_ins, tc.bits(tv, n), tc.bits(ti, n), mixed)
    assert not got_ins[~defined].any()
    # the sweep: undefined local boxes stay undefined through the identity (0 * Inf is NaN); the rule decides from the world boxes
    ents = tc.identity_entities(mixed)
    sw = EcsSweep(ctx, ents, trace="octree")
    _, a, v = sw.run(planes[3])
    ctx.synchronize()
    _, oa, _ = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes[3])
    np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), oa.view(np.uint32))
    # (AABB::Apply's comparisons drop a NaN that only one corner of the last pair sees, and its FLT_MIN seed of the max turns the -3e9 box into
    # [-3e9, FLT_MIN]: defined, but beyond the oracle's int32 arithmetic -- held against the rule only)
    rv, ri, wdef = tc.trace_rule(oa, planes[3], root)
    keep = tc.oracle_comparable(oa)
    assert (~wdef).sum() >= len(tc.UNDEFINED) - 2 and (~keep).sum() > (~wdef).sum()
    tv, ti, _, _ = oracle.trace_scene_octree_boxes(tc.oracle_safe(oa, keep, root), planes[3])
    got_v, got_i = tc.bits(u64(v), n), tc.bits(u64(sw.inserted), n)
    assert not got_v[~wdef].any() and not got_i[~wdef].any()
    np.testing.assert_array_equal(got_v[keep], tc.bits(tv, n)[keep])
    np.testing.assert_array_equal(got_i[keep], tc.bits(ti, n)[keep])
    np.testing.assert_array_equal(got_v, rv)
    np.testing.assert_array_equal(got_i, ri)


@pytest.mark.parametrize("world, count", [(2, 100000), (3, 100000), (8, 100000), (2, 1 << 20), (3, 1 << 20), (8, 1 << 20)])
def test_octree_slices_are_the_whole_sweeps_words(ctx, world, count):
    """every rank's slice in octree mode, laid side by side as the all-gather lays them: the whole octree-mode sweep's visibility and inserted words"""
    ents = synth.make_entities(count)
    planes = camera_planes(synth.make_camera(3840, 2160))
    whole = EcsSweep(ctx, ents, trace="octree")
    _, _, wv = whole.run(planes)
    ctx.synchronize()
    wv, wi = u64(wv), u64(whole.inserted)
    words = (count + 63) // 64
    vis, ins = [], []
    for r in range(world):
        sw = EcsSweep(ctx, ents, rank=r, world=world, trace="octree")
        sw.visibility.fill_(-1); sw.inserted.fill_(-1)
        _, _, v = sw.run(planes)
        ctx.synchronize()
        v, i = u64(v), u64(sw.inserted)
        slot = slice(r * sw.words_per_rank, (r + 1) * sw.words_per_rank)
        vis.append(v[slot]); ins.append(i[slot])
        lo_w, hi_w = sw.begin // 64, (sw.end + 63) // 64
        assert (v[:lo_w] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (v[hi_w:words] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "only the slice's bits"
        assert (i[:lo_w] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (i[hi_w:words] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "only the slice's bits"
    # (the fill's bits past the last entity stay: compare the entities' bits)
    np.testing.assert_array_equal(tc.bits(np.concatenate(vis), count), tc.bits(wv, count))
    np.testing.assert_array_equal(tc.bits(np.concatenate(ins), count), tc.bits(wi, count))


@pytest.mark.parametrize("levels", [5, 9])
def test_octree_mode_of_a_deep_hierarchy(ctx, levels):
    """more than four levels: one launch per level, words straddling level boundaries completed by two launches -- visibility and inserted words"""
    per, n = 37 + 64 * 3, 0
    ents = synth.make_entities(per * levels, editor_world=False)
    offs = [0]
    for lvl in range(levels):
        n += per + 5 * lvl
        offs.append(min(n, per * levels))
    offs[-1] = per * levels
    ents.level_offsets = np.array(offs, np.uint32)
    ents.parent[:] = 0xFFFFFFFF
    u = synth.uniforms(synth.STREAM_ENTITIES, per * levels, 1 << 26)
    for lvl in range(1, levels):
        lo, hi, plo, phi = offs[lvl], offs[lvl + 1], offs[lvl - 1], offs[lvl]
        ents.parent[lo:hi] = (plo + np.floor(u[lo:hi] * (phi - plo))).astype(np.uint32)
        ents.transforms[lo:hi, 0:3] *= np.float32(0.05)
        ents.transforms[lo:hi, 8:11] = np.float32(0.9) + np.float32(0.2) * ents.transforms[lo:hi, 8:11] / np.float32(4.0)
    planes = camera_planes(synth.make_camera(1920, 1080))
    sw = EcsSweep(ctx, ents, trace="octree")
    w, a, v = sw.run(planes)
    ctx.synchronize()
    ow, oa, _ = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes)
    tv, ti, _, _ = oracle.trace_scene_octree_boxes(oa, planes)
    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), ow.view(np.uint32))
    np.testing.assert_array_equal(u64(v), tv)
    np.testing.assert_array_equal(u64(sw.inserted), ti)
    assert 0 < popcount(tv) < per * levels


def test_cascade_mesh_lists_through_the_octree(ctx):
    """LightingECS.cpp:296 TraceScene(frustums[k], true) over the 2^20 sweep's world boxes and four cascade frusta (as
    test_cascade_caster_sets_from_the_sweeps_world_boxes builds them): each cascade's mask is the octree's; then 1 000 entities and two cascades"""
    ents = synth.make_entities(1 << 20)
    cam = synth.make_camera(3840, 2160)
    _, aabb, _ = EcsSweep(ctx, ents).run(camera_planes(cam))
    sh = synth.make_shadow_set(cam, 16)
    planes = np.stack([host.extract_frustum_planes_matrix(sh.lights_matrices[k])[0] for k in range(4)])
    for m, k in ((1 << 20, 4), (1000, 2)):
        ins = torch.zeros(((m + 63) // 64,), dtype=torch.int64, device=ctx.device)
        got = csm_caster_masks(ctx, aabb[:m], planes[:k], trace="octree", inserted=ins)
        ctx.synchronize()
        boxes = aabb[:m].cpu().numpy()
        for c in range(k):
            tv, ti, _, _ = oracle.trace_scene_octree_boxes(boxes, planes[c])
            np.testing.assert_array_equal(u64(got[c]), tv)
            np.testing.assert_array_equal(u64(ins), ti)
        if m == 1 << 20:
            counts = [popcount(u64(got[c])) for c in range(k)]
            assert 0 < counts[0] < counts[3] < m


def test_invalid_traces_are_refused(ctx):
    lib = _lib.load()
    boxes = torch.zeros((64, 6), dtype=torch.float32, device=ctx.device)
    masks = torch.zeros((1, 1), dtype=torch.int64, device=ctx.device)
    ins = torch.zeros(2, dtype=torch.int64, device=ctx.device)
    pl = np.ascontiguousarray(tc.camera_planes())
    fp = pl.ctypes.data_as(C.POINTER(C.c_float))
    for mode, root, dins in ((7, 0, None), (_lib.TRACE_OCTREE_INT_BOXES, 1, None), (_lib.TRACE_OCTREE_INT_BOXES, (1 << 30) + 2, None),
                             (_lib.TRACE_FLAT_FLOAT_BOXES, 0, ins.data_ptr()), (_lib.TRACE_OCTREE_INT_BOXES, 0, ins.data_ptr() + 4)):
        tr = _lib.SceneTrace(mode, root, dins)
        assert lib.sailor_hip_csm_caster_masks_traced(ctx.handle, 64, boxes.data_ptr(), fp, 1, masks.data_ptr(), C.byref(tr)) == -1
    ents = synth.make_entities(64)
    sw = EcsSweep(ctx, ents, trace="octree")
    sw._trace.mode = 9
    with pytest.raises(_lib.SailorHipError) as e:
        sw.run(pl)
    assert e.value.status == -1


def test_the_runtime_sweep_in_octree_mode(ctx):
    """EcsSweepSystem with its trace mode set, through sailor_rt_ecs_sweep_traced and the scene view's camera: the octree's words; flat mode through
    the same entry point is sailor_hip_ecs_sweep's"""
    from sailor_amd.runtime_binding import Runtime
    cam = synth.make_camera(1280, 720)
    ents = synth.make_entities(5000)
    planes = camera_planes(cam)
    _, oa, ov = oracle.ecs_sweep(ents.transforms, ents.parent, ents.local_aabb, planes)
    tv, ti, _, _ = oracle.trace_scene_octree_boxes(oa, planes)
    lib = _lib.load()
    n = len(ents.parent)
    words = (n + 63) // 64

    def download(ptr, count):
        out = np.empty(count, np.uint64)
        _lib.check(lib.sailor_hip_buffer_download(ctx.handle, out.ctypes.data, ptr, 0, out.nbytes), "buffer_download", ctx.handle)
        return out

    rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
    try:
        rt.set_camera(cam)
        st, _, a, v, ins = rt.ecs_sweep_traced(ents, "octree")
        assert st == 0 and ins
        rt.wait_idle()
        np.testing.assert_array_equal(download(a, len(oa) * 3).view(np.uint32), oa.reshape(-1).view(np.uint32))
        np.testing.assert_array_equal(tc.bits(download(v, words), n), tc.bits(tv, n))   # (the entities' bits: the sweep leaves the rest)
        np.testing.assert_array_equal(download(ins, words), ti)                           # SetTraceMode cleared the words: padding is 0
        st, _, _, v, ins = rt.ecs_sweep_traced(ents, "flat")
        assert st == 0 and ins is None
        rt.wait_idle()
        np.testing.assert_array_equal(tc.bits(download(v, words), n), tc.bits(ov, n))
    finally:
        rt.close()
