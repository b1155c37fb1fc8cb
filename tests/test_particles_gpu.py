"""ExperimentalParticles through the C-ABI (sailor_amd/csrc/particles.hip) against tests/particles_ref.py.

Update: integer fields, the exact-by-construction entries and the sentinels bit for bit against the fp32 restatement; matrices and colours of the generic
instances against float64 within GPU_BOUND_FACTOR x E_REF.  Shadow map: fed with the instance buffer the GPU update produced, bit for bit over the whole map.
Colour pass: fed with that buffer and the GPU's own map; coverage, the owning primitive and DepthBuffer bit for bit, Main bit for bit outside coverage and
within 1e-4 relative of float64 inside it wherever float64 decides the fragment's discrete steps (elsewhere: one of the outcomes float64 allows).
Observed on an MI355X (printed by the tests): see GPU_OBSERVED_* in tests/particles_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import particles_cases as cases
import particles_ref as ref
from particles_run import Device, dev, frame_of, gpu_update
from sailor_amd import _lib

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ROTATION = [0, 1, 2, 4, 5, 6, 8, 9, 10]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("name", list(cases.UPDATE_CASES))
def test_update(ctx, name):
    c = cases.UPDATE_CASES[name]()
    got = gpu_update(ctx, c)
    o32, o64 = ref.update(c["records"], c["pc"], c["time"], f32), ref.update(c["records"], c["pc"], c["time"], f64)
    want = ref.apply_update(c["before"], o32)
    # integer fields and what the kernel must not write (U7)
    np.testing.assert_array_equal(got["isCulled"], want["isCulled"])
    assert (got["materialInstance"] == cases.SENTINEL).all() and (got["_pad"] == cases.SENTINEL).all()
    # exact by construction: the translation column everywhere; the whole matrix where the rotation is the identity (the gate is closed) and no decay
    # enters the scale; a zero record's; the colours' rgb everywhere and their alpha wherever the decay is exactly 1
    np.testing.assert_array_equal(bits(got["model"][:, 12:16]), bits(want["model"][:, 12:16]))
    closed = ~o32["gate"]
    np.testing.assert_array_equal(bits(got["model"][closed]), bits(want["model"][closed]))
    np.testing.assert_array_equal(bits(got["model"][o32["zero_new"]]), bits(np.tile(np.array([0] * 15 + [1], f32), (int(o32["zero_new"].sum()), 1))))
    np.testing.assert_array_equal(bits(got["color"][:, :3]), bits(want["color"][:, :3]))
    np.testing.assert_array_equal(bits(got["colorOld"][:, :3]), bits(want["colorOld"][:, :3]))
    plain = (o32["current"] == 0) | (float(c["pc"].traceDecay) == 1.0)                   # pow(x, 0) = pow(1, y) = 1 in any library
    np.testing.assert_array_equal(bits(got["color"][plain]), bits(want["color"][plain]))
    np.testing.assert_array_equal(bits(got["colorOld"][plain]), bits(want["colorOld"][plain]))
    # the generic instances against float64: every entry
    g = ref.generic(o64)
    if g.any():
        dm = ref.deviation(got["model"][g], o64["model"][g]).max()
        dc = max(ref.deviation(got["color"][g], o64["color"][g]).max(), ref.deviation(got["colorOld"][g], o64["colorOld"][g]).max())
        print(f"{name}: {int(g.sum())} generic instances, matrix {dm:.3f}, colour {dc:.3f} (x 2^-23 x the largest magnitude)")
        assert dm <= ref.GPU_BOUND_FACTOR * ref.E_REF_MATRIX and dc <= ref.GPU_BOUND_FACTOR * ref.E_REF_COLOUR
    if name == "U3_placed":
        # +up, -up, one ulp off up, along x, along y, p1 == p2: the structural facts
        assert o32["gate"].tolist() == [False, False, True, True, True, False]
        m = got["model"]
        assert m[1][10] == 2 and m[1][0] == m[1][5] == f32(0.75)                       # -up is not flipped
        assert m[5][10] == 0 and m[5][0] == f32(0.75) and np.isfinite(m[5]).all()      # p1 == p2: the identity and a zz scale of 0
        np.testing.assert_array_equal(bits(m[2]), bits(want["model"][2]))              # one ulp off up: acos(1) = 0, cos 1, sin 0 in any library
        for k, axis in ((3, 0), (4, 1)):                                               # along x / y: the box's long axis lands on x / y
            long = m[k][8:11]
            assert abs(long[axis]) == pytest.approx(1.5, rel=1e-6) and np.abs(np.delete(long, axis)).max() < 1e-6


@pytest.fixture(scope="module")
def rendered(ctx):
    """update -> shadow -> draw on the device, the restatements over what the device produced"""
    s = cases.pass_scene()
    d = Device(ctx, s)
    _lib.check(d.update(), "sailor_hip_particles_update", ctx.handle)
    ctx.synchronize()
    inst = d.download_instances()
    pre = cases.prepass_depth(s, inst, ref)
    d.depth.copy_(torch.from_numpy(pre))
    _lib.check(d.shadow(), "sailor_hip_particles_shadow", ctx.handle)
    _lib.check(d.colour(), "sailor_hip_particles_draw", ctx.handle)
    ctx.synchronize()
    out = dict(scene=s, device=d, inst=inst, pre=pre, map=d.map.cpu().numpy(), main=d.main.cpu().numpy(), depth=d.depth.cpu().numpy(),
               keys=d.workspace.cpu().numpy().view(np.uint64)[: cases.W * cases.H].reshape(cases.H, cases.W).copy())
    out["smap"] = ref.raster(inst["model"], s["vertices"], s["indices"], cases.MAP_W, cases.MAP_H, light_matrix=s["light_matrix"])
    out["colour"] = ref.raster(inst["model"], s["vertices"], s["indices"], cases.W, cases.H, projection=s["projection"], view=s["view"], depth0=pre)
    return out


def test_pass_scene_instances(rendered):
    s, inst = rendered["scene"], rendered["inst"]
    o32 = ref.update(s["records"], s["pc"], s["time"], f32)
    want = ref.apply_update(s["before"], o32)
    assert (inst["materialInstance"] == 3).all() and (inst["_pad"] == 0).all()
    closed = ~o32["gate"]
    assert closed.tolist() == [True, True, True, False, True, False, False]
    np.testing.assert_array_equal(bits(inst["model"][closed]), bits(want["model"][closed]))
    np.testing.assert_array_equal(bits(inst["color"]), bits(want["color"]))
    np.testing.assert_array_equal(bits(inst["colorOld"]), bits(want["colorOld"]))


def test_shadow_map_bit_for_bit(rendered):
    got, want = rendered["map"], rendered["smap"]
    np.testing.assert_array_equal(bits(got), bits(want["map"]))
    assert (got[want["owner"] == 0] == 0).all() and want["stats"]["later_farther"] >= 40
    under = (want["owner"].astype(int) - 1) // 24 == 1
    assert under.sum() > 80 and np.allclose(got[under & (want["owner"] != 0)], 0.425, atol=1e-6)     # the later, farther cube's depth: order over depth


def test_colour_pass(rendered):
    s, want, pre = rendered["scene"], rendered["colour"], rendered["pre"]
    owner = (rendered["keys"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    np.testing.assert_array_equal(owner, want["owner"])                                  # coverage and the owning primitive
    np.testing.assert_array_equal(bits(rendered["depth"]), bits(want["depth"]))
    cov = want["owner"] != 0
    assert (bits(rendered["depth"])[~cov] == bits(pre)[~cov]).all()
    np.testing.assert_array_equal(bits(rendered["main"])[~cov], bits(s["main0"])[~cov])
    assert want["stats"]["ties"] >= 12 and want["stats"]["depth_failed"] >= 20 and want["stats"]["cut_one"] > 0 and want["stats"]["cut_two"] > 0
    r64 = ref.shade(want, rendered["inst"], s["vertices"], s["lights"]["direction"][0], s["light_matrix"], s["projection"], s["view"], rendered["map"], s["main0"], T=f64)
    und = ref.undecided(r64)
    ok = ref.within(rendered["main"], r64["main"]).all(-1)
    with np.errstate(all="ignore"):
        rel = np.abs(rendered["main"].astype(f64) - r64["main"]) / np.abs(r64["main"])
    print(f"covered {int(cov.sum())}, undecided {int(und.sum())}, worst relative error on decided pixels {np.nanmax(rel[cov & ~und]):.3e}")
    assert und.sum() <= ref.MAX_UNDECIDED_FRACTION * cov.sum()
    assert ok[cov & ~und].all(), np.argwhere(cov & ~und & ~ok)[:5].tolist()
    allowed = ref.within(rendered["main"][None], ref.allowed_outcomes(r64)).all(-1).any(0)
    assert allowed[und].all()


def test_swapped_map_extents_show(ctx, rendered):
    s = rendered["scene"]
    d = Device(ctx, s, map_w=cases.MAP_H, map_h=cases.MAP_W)
    d.instances.copy_(rendered["device"].instances)
    _lib.check(d.shadow(), "sailor_hip_particles_shadow", ctx.handle)
    ctx.synchronize()
    want = ref.raster(rendered["inst"]["model"], s["vertices"], s["indices"], cases.MAP_H, cases.MAP_W, light_matrix=s["light_matrix"])
    np.testing.assert_array_equal(bits(d.map.cpu().numpy()), bits(want["map"]))


def test_refusals_leave_the_outputs_untouched(ctx):
    s = cases.pass_scene()
    lib = ctx._lib
    d = Device(ctx, s)
    inst0, map0, main0, depth0 = d.instances.clone(), d.map.clone(), d.main.clone(), d.depth.clone()
    pc = s["pc"]

    def constants(**kw):
        v = dict(numInstances=pc.numInstances, numFrames=pc.numFrames, fps=pc.fps, traceFrames=pc.traceFrames, traceDecay=pc.traceDecay)
        v.update(kw)
        return _lib.ParticlesConstants(**v)

    def update(c=None, frame=None, records=None, instances=None):
        return lib.sailor_hip_particles_update(ctx.handle, C.byref(frame or d.frame), C.byref(c or pc), d.records.data_ptr() if records is None else records,
                                               len(s["records"]), d.instances.data_ptr() if instances is None else instances)
    assert update(records=0) == -1 and update(instances=0) == -1
    assert update(records=d.records.data_ptr() + 4) == -1 and update(instances=d.instances.data_ptr() + 8) == -1
    assert update(instances=d.records.data_ptr() + 80) == -1 and b"overlap" in lib.sailor_hip_context_last_error(ctx.handle)
    assert update(constants(numInstances=2 ** 31)) == -1 and update(constants(numInstances=2 ** 32 - 1)) == -1
    assert update(constants(numInstances=0)) == -1 and update(constants(traceFrames=0)) == -1 and update(constants(numFrames=0)) == -1
    for decay in (0.0, -0.5, float("inf"), float("nan")):
        assert update(constants(traceDecay=decay)) == -1
    for time in (-1.0, float("inf"), float("nan")):
        assert update(frame=frame_of(time)) == -1
    assert update(constants(fps=4000000000), frame=frame_of(3e38)) == -1

    def shadow(draw=None, instances=None, n=None, matrices=None, smap=None, w=cases.MAP_W, h=cases.MAP_H, ws=None, nbytes=None):
        return lib.sailor_hip_particles_shadow(ctx.handle, C.byref(draw or d.draw), d.instances.data_ptr() if instances is None else instances, d.n if n is None else n,
                                               d.matrices.data_ptr() if matrices is None else matrices, d.map.data_ptr() if smap is None else smap, w, h,
                                               d.workspace.data_ptr() if ws is None else ws, d.bytes if nbytes is None else nbytes)

    def colour(draw=None, instances=None, n=None, lights=None, matrices=None, smap=None, mw=cases.MAP_W, mh=cases.MAP_H, main=None, depth=None, w=cases.W, h=cases.H,
               ws=None, nbytes=None):
        return lib.sailor_hip_particles_draw(ctx.handle, C.byref(d.frame), C.byref(draw or d.draw), d.instances.data_ptr() if instances is None else instances,
                                             d.n if n is None else n, d.lights.data_ptr() if lights is None else lights,
                                             d.matrices.data_ptr() if matrices is None else matrices, d.map.data_ptr() if smap is None else smap, mw, mh,
                                             d.main.data_ptr() if main is None else main, d.depth.data_ptr() if depth is None else depth, w, h,
                                             d.workspace.data_ptr() if ws is None else ws, d.bytes if nbytes is None else nbytes)
    no_mesh = _lib.ParticlesDraw(dVertices=0, dIndices=d.indices.data_ptr(), numTriangles=12)
    no_triangles = _lib.ParticlesDraw(dVertices=d.vertices.data_ptr(), dIndices=d.indices.data_ptr(), numTriangles=0)
    many = _lib.ParticlesDraw(dVertices=d.vertices.data_ptr(), dIndices=d.indices.data_ptr(), numTriangles=(2 ** 32 - 1 + 13) // 14)
    for call in (shadow, colour):
        assert call(draw=no_mesh) == -1 and call(draw=no_triangles) == -1 and call(n=0) == -1 and call(instances=0) == -1 and call(instances=d.instances.data_ptr() + 4) == -1
        assert call(matrices=0) == -1 and call(smap=0) == -1 and call(ws=0) == -1 and call(ws=d.workspace.data_ptr() + 8) == -1
        assert call(draw=many, n=7) == -1 and b"2^32 - 1" in lib.sailor_hip_context_last_error(ctx.handle)
        assert call(ws=d.instances.data_ptr()) == -1                                                      # overlapping in and out
    assert shadow(smap=d.instances.data_ptr()) == -1 and colour(main=d.instances.data_ptr()) == -1
    assert shadow(w=0) == -1 and shadow(h=32769) == -1 and shadow(nbytes=8 * cases.MAP_W * cases.MAP_H - 8) == -1
    assert shadow(smap=d.workspace.data_ptr()) == -1
    assert colour(w=0) == -1 and colour(h=32769) == -1 and colour(mw=0) == -1 and colour(nbytes=8 * cases.W * cases.H - 8) == -1
    assert colour(lights=0) == -1 and colour(main=0) == -1 and colour(depth=0) == -1 and colour(main=d.main.data_ptr() + 4) == -1
    assert colour(main=d.map.data_ptr()) == -1 and colour(depth=d.main.data_ptr()) == -1 and colour(depth=d.workspace.data_ptr()) == -1
    ctx.synchronize()
    assert torch.equal(d.instances, inst0) and torch.equal(d.map, map0) and torch.equal(d.main, main0) and torch.equal(d.depth, depth0)
    assert (d.workspace == -1).all()


def test_update_shadow_draw_in_a_captured_graph(rendered):
    """the three calls record only: captured on one stream and replayed over cleared outputs, they give the eager run's bytes"""
    from sailor_amd.forward_plus import HipContext
    s = rendered["scene"]
    side = torch.cuda.Stream()
    ctx = HipContext("cuda:0", stream=side)
    try:
        with torch.cuda.stream(side):
            d = Device(ctx, s)
            pre = torch.from_numpy(rendered["pre"]).to(ctx.device)
            main0, before = d.main.clone(), d.instances.clone()
            d.depth.copy_(pre)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            assert d.update() == 0 and d.shadow() == 0 and d.colour() == 0
        for _ in range(2):
            d.instances.copy_(before); d.main.copy_(main0); d.depth.copy_(pre); d.map.fill_(-7.0)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(d.instances.cpu().numpy(), rendered["device"].instances.cpu().numpy())
            np.testing.assert_array_equal(bits(d.map.cpu().numpy()), bits(rendered["map"]))
            np.testing.assert_array_equal(bits(d.main.cpu().numpy()), bits(rendered["main"]))
            np.testing.assert_array_equal(bits(d.depth.cpu().numpy()), bits(rendered["depth"]))
        del g
    finally:
        torch.cuda.synchronize()
        ctx.close()
