"""The torch-facing binding against a recording stand-in for libsailor_hip.so, on CPU tensors: which C-ABI entries every route of SurfacePass, ForwardPlus and
EcsSweep calls, in which order and with which scalar arguments.

The stand-in folds the three forwarder families the way the C does (shade.hip, light_cull.hip, ecs_sweep.hip): sailor_hip_shade and _ex record as _prepared
with the missing arguments NULL or 0, sailor_hip_light_cull as _prepared, sailor_hip_ecs_sweep and _range as _traced.  What is asserted here is therefore the
call the library's one body sees, whichever entry the binding chose to reach it through."""
import ctypes as C

import numpy as np
import pytest
import torch

from sailor_amd import _lib, synth
from sailor_amd.forward_plus import EcsSweep, ForwardPlus, HipContext, PreparedLights, SurfacePass

W, H = 32, 16
BYTES = 4096                                        # every _bytes / _size query
TILE_ORDER, TILE_NUM, TILE_LISTS = 0x1000, 0x2000, 0x3000  # the pointers the tile-list queries give
GLTF, CUTOUT, BACK = _lib.SURFACE_GLTF, _lib.SURFACE_ALPHA_CUTOUT, _lib.SURFACE_CULL_BACK


class RecordingLib:
    """sailor_hip_* attributes that append (name, context handle, arguments) to `calls` and return 0.  Host arithmetic that needs no device goes to the real
    library; the size and tile-order queries answer fixed values and are not recorded."""
    REAL = {"sailor_hip_num_tiles", "sailor_hip_band_whole_frame", "sailor_hip_band_from_tile_rows", "sailor_hip_surface_draw_prims", "sailor_hip_ecs_range_for_rank",
            "sailor_hip_status_string"}

    def __init__(self, real):
        self.real, self.calls, self.commits = real, [], None

    def __getattr__(self, name):
        if not name.startswith("sailor_"):
            raise AttributeError(name)
        if name in self.REAL or name.startswith("sailor_host_"):
            return getattr(self.real, name)
        if name.endswith("_bytes") or name.endswith("_size"):
            return lambda *a: BYTES
        if name == "sailor_hip_light_cull_tile_order":
            return lambda *a: TILE_ORDER
        if name == "sailor_hip_context_destroy":
            return lambda *a: 0
        return lambda *a: self._record(name, *a)

    def _record(self, name, *a):
        if name == "sailor_hip_light_cull_tile_lists":   # (no context: a query)
            a[-2]._obj.value, a[-1]._obj.value = TILE_NUM, TILE_LISTS
            return 0
        handle, a = a[0], a[1:]
        if name == "sailor_hip_shade":         # (…, csm, out, band) -> (…, csm, ibl = NULL, out, band, order = NULL)
            name, a = "sailor_hip_shade_ex", a[:8] + (None,) + a[8:] + (None,)
        if name == "sailor_hip_shade_ex":
            name, a = "sailor_hip_shade_prepared", a + (None, 0)
        if name == "sailor_hip_light_cull":
            name, a = "sailor_hip_light_cull_prepared", a + (None, 0)
        if name == "sailor_hip_ecs_sweep":     # (n, …) -> (n, …, 0, n)
            name, a = "sailor_hip_ecs_sweep_range", a + (0, a[0])
        if name == "sailor_hip_ecs_sweep_range":
            name, a = "sailor_hip_ecs_sweep_traced", a + (None,)
        if name == "sailor_hip_surface_peel_commit" and self.commits:   # the committed pixels the test asks for, where the binding reads them
            C.c_int32.from_address(a[6]).value = self.commits.pop(0)
        self.calls.append((name, handle, a))
        return 0

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@pytest.fixture()
def lib(monkeypatch):
    stand_in = RecordingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", stand_in)   # what _lib.load() returns
    return stand_in


def make_ctx(lib, handle=1):
    ctx = HipContext.__new__(HipContext)
    ctx.device, ctx.stream, ctx.handle, ctx._lib = torch.device("cpu"), None, handle, lib
    return ctx


def names(calls):
    return [c[0] for c in calls]


def desc(call):
    """(primBase, flags, numTriangles, numDrawn, firstInstance) of the SailorSurfaceDraw a draw entry was handed"""
    d = call[2][1]._obj
    return d.primBase, d.flags, d.numTriangles, d.numDrawn, d.firstInstance


# ---- SurfacePass ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def scene():
    z = lambda n: torch.zeros(n, dtype=torch.uint8)
    return dict(vertices=z(72 * 6), indices=torch.zeros(6, dtype=torch.int32), instances=z(96 * 3), materials=z(80 * 2), textures=z(64))


def test_draw_takes_one_of_four_entries(lib, scene):
    sp = SurfacePass(make_ctx(lib), W, H)
    frame = _lib.UboFrameData()
    sp.begin(prim_base=5)
    tables = dict(materials=scene["materials"], textures=scene["textures"], num_textures=2)
    sp.draw(frame, scene["vertices"], scene["indices"], scene["instances"], cull_back=True)
    sp.draw(frame, scene["vertices"], scene["indices"], scene["instances"], alpha_cutout=True, first_instance=1, **tables)
    sp.draw(frame, scene["vertices"], scene["indices"], scene["instances"], gltf=True, num_drawn=2, **tables)
    sp.draw(frame, scene["vertices"], scene["indices"], scene["instances"], lod=True, instance_ids=torch.zeros(4, dtype=torch.int32), **tables)
    calls = lib.take()
    assert names(calls) == ["sailor_hip_surface_begin", "sailor_hip_surface_draw", "sailor_hip_surface_draw_masked", "sailor_hip_surface_draw_gltf",
                            "sailor_hip_surface_draw_lod"]
    # 2 triangles a draw; the instances tensor holds 3 records; primBase advances by sailor_hip_surface_draw_prims: 2 a triangle and instance
    assert [desc(c) for c in calls[1:]] == [(5, BACK, 2, 3, 0), (17, CUTOUT, 2, 2, 1), (25, GLTF, 2, 2, 0), (33, 0, 2, 4, 0)]
    assert calls[1][2][3] == 0 and [c[2][7] for c in calls[2:]] == [1, 2, 3]                      # the draw index
    assert calls[1][2][4:6] == (W, H) and all(c[2][8:10] == (W, H) and c[2][4] == 2 and c[2][6] == 2 for c in calls[2:])  # extent; 2 materials, 2 textures
    tables_of = (scene["instances"].data_ptr(), scene["materials"].data_ptr(), scene["textures"].data_ptr())   # each table in its own argument
    assert calls[1][2][2] == tables_of[0] and all((c[2][2], c[2][3], c[2][5]) == tables_of for c in calls[2:])
    assert (sp.prim_base, sp.draw_index) == (49, 4)


def test_draw_indirect_takes_one_of_two_entries(lib, scene):
    sp = SurfacePass(make_ctx(lib), W, H)
    frame = _lib.UboFrameData()
    command = torch.zeros(10, dtype=torch.int32)
    sp.begin()
    sp.draw_indirect(frame, scene["vertices"], scene["indices"], scene["instances"], command, capacity=3, command_index=1, cull_back=True)
    sp.draw_indirect(frame, scene["vertices"], scene["indices"], scene["instances"], command, capacity=2, num_instance_records=2, alpha_cutout=True, lod=True,
                     materials=scene["materials"], textures=scene["textures"], num_textures=2)
    calls = lib.take()
    assert names(calls) == ["sailor_hip_surface_begin", "sailor_hip_surface_draw_indirect", "sailor_hip_surface_draw_indirect_lod"]
    assert [desc(c) for c in calls[1:]] == [(0, BACK, 2, 3, 0), (12, CUTOUT, 2, 2, 0)]
    assert [c[2][2] - command.data_ptr() for c in calls[1:]] == [20, 0]                            # the command
    assert [(c[2][4], c[2][6], c[2][8], c[2][9]) for c in calls[1:]] == [(3, 0, 0, 0), (2, 2, 2, 1)]   # instance records, materials, textures, draw index
    assert (sp.prim_base, sp.draw_index) == (20, 2)


def two_draws(scene):
    """one Standard and one glTF draw with distinct blend modes"""
    return [dict(vertices=scene["vertices"], indices=scene["indices"], blend="additive", cull_back=True),
            dict(vertices=scene["vertices"], indices=scene["indices"], blend="alpha", gltf=True, num_drawn=1, first_instance=2)]


def blend_bits(mode):
    return _lib.SURFACE_BLEND_MODES[mode] << _lib.SURFACE_BLEND_SHIFT


def run_transparent(lib, scene, **kw):
    sp = SurfacePass(make_ctx(lib), W, H)
    seen = []
    target, depth = torch.zeros(H, W, 4), torch.zeros(H, W)
    counts = sp.transparent(_lib.UboFrameData(), two_draws(scene), scene["instances"], scene["materials"], scene["textures"], 2, depth,
                            lambda s, ao: torch.zeros(H, W, 4), target, prim_base=7, on_layer=lambda k, *a: seen.append((k, a[2] is not None, a[3] is not None)), **kw)
    return sp, lib.take(), counts, seen


PEEL_ROUND = ["sailor_hip_surface_peel_begin", "sailor_hip_surface_peel_draw", "sailor_hip_surface_peel_draw_gltf", "sailor_hip_surface_peel_commit"]
LAYER_END = ["sailor_hip_surface_resolve_gltf", "sailor_hip_surface_blend"]   # (a pass with a glTF draw resolves through resolve_gltf; the shade is the caller's)


def test_transparent_peel_with_a_budget(lib, scene):
    sp, calls, counts, seen = run_transparent(lib, scene, mode="peel", layers=2)
    assert names(calls) == (PEEL_ROUND + LAYER_END) * 2 + PEEL_ROUND
    draws = [c for c in calls if "peel_draw" in c[0]]
    assert [desc(c) for c in draws] == [(7, BACK | blend_bits("additive"), 2, 3, 0), (19, GLTF | blend_bits("alpha"), 2, 1, 2)] * 3
    assert [c[2][7] for c in draws] == [0, 1] * 3                                                  # the draw index
    tables_of = (scene["instances"].data_ptr(), scene["materials"].data_ptr(), scene["textures"].data_ptr())
    assert all((c[2][2], c[2][3], c[2][5]) == tables_of for c in draws)
    assert all((c[2][1], c[2][2], c[2][4]) == tables_of for c in calls if c[0].endswith("resolve_gltf"))   # (frame, instances, materials, count, textures, …)
    assert [c[2][6] for c in calls if c[0].endswith("peel_begin")] == [1, 0, 0]                    # only layer 0 clears `last`
    assert seen == [(0, True, True), (1, True, True)] and tuple(counts.shape) == (3,)
    assert (sp.prim_base, sp.draw_index) == (23, 2)


def test_transparent_buckets(lib, scene):
    sp, calls, counts, seen = run_transparent(lib, scene, mode="buckets", layers=2)
    layer = ["sailor_hip_surface_bucket_layer"]
    assert names(calls) == ["sailor_hip_surface_bucket_begin", "sailor_hip_surface_bucket_draw", "sailor_hip_surface_bucket_draw_gltf"] + \
                           (layer + LAYER_END) * 2 + layer
    assert [desc(c) for c in calls[1:3]] == [(7, BACK | blend_bits("additive"), 2, 3, 0), (19, GLTF | blend_bits("alpha"), 2, 1, 2)]
    assert [c[2][7] for c in calls[1:3]] == [0, 1] and [c[2][15:17] for c in calls[1:3]] == [(BYTES, 2)] * 2   # draw index; the store's bytes and layers
    assert calls[0][2][6:8] == (BYTES, 2)
    assert [c[2][6:9] for c in calls if c[0].endswith("bucket_layer")] == [(BYTES, 2, 0), (BYTES, 2, 1), (BYTES, 2, 2)]   # bytes, layers, k
    assert seen == [(0, True, True), (1, True, True)] and tuple(counts.shape) == (3,)
    assert (sp.prim_base, sp.draw_index) == (23, 2)


def test_transparent_without_a_budget_stops_at_the_first_empty_layer(lib, scene):
    lib.commits = [9, 4, 0]
    sp, calls, counts, seen = run_transparent(lib, scene, layers=None)
    peel = PEEL_ROUND + ["sailor_hip_context_synchronize"]
    assert names(calls) == (peel + LAYER_END) * 2 + peel
    assert counts.tolist() == [9, 4, 0] and [k for k, *_ in seen] == [0, 1]


def test_multisampled(lib, scene):
    sp = SurfacePass(make_ctx(lib), W, H)
    seen = []
    sp.multisampled(_lib.UboFrameData(), two_draws(scene), scene["instances"], scene["materials"], scene["textures"], 2, lambda s, ao: torch.zeros(H, W, 4),
                    torch.zeros(H, W, 4), samples=4, layers=2, prim_base=7, on_layer=lambda k, s, weight, *a: seen.append((k, weight.data_ptr())))
    calls = lib.take()
    layer = ["sailor_hip_surface_msaa_layer", "sailor_hip_surface_resolve_gltf", "sailor_hip_surface_msaa_accumulate"]
    assert names(calls) == ["sailor_hip_surface_msaa_begin", "sailor_hip_surface_msaa_draw", "sailor_hip_surface_msaa_draw_gltf"] + layer * 2
    assert [desc(c) for c in calls[1:3]] == [(7, BACK, 2, 3, 0), (19, GLTF, 2, 1, 2)]              # no blend bits: the pass has no blending
    assert calls[0][2][6:8] == (BYTES, 4) and [c[2][7] for c in calls[1:3]] == [0, 1] and [c[2][14:16] for c in calls[1:3]] == [(BYTES, 4)] * 2
    layers = [c for c in calls if c[0].endswith("msaa_layer")]
    assert [c[2][6:10] for c in layers] == [(BYTES, 4, 2, 0), (BYTES, 4, 2, 1)]                    # bytes, samples, layers, k
    assert [c[2][11] is not None for c in layers] == [True, False]                                 # the uncovered bytes are written by layer 0
    assert [c[2][4:6] for c in calls if c[0].endswith("accumulate")] == [(4, 0), (4, 1)]           # samples, k
    assert seen == [(0, sp.weights[0].data_ptr()), (1, sp.weights[1].data_ptr())]
    assert (sp.prim_base, sp.draw_index, sp.samples) == (23, 2, 4)


# ---- ForwardPlus ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ibl", [False, True])
@pytest.mark.parametrize("tile_lists", [False, True])
@pytest.mark.parametrize("with_prepared", [False, True])
def test_cull_and_shade(lib, with_prepared, tile_lists, with_ibl):
    f = synth.make_frame("tiny")
    w, h, n = f.cam.width, f.cam.height, len(f.lights)
    own, other = make_ctx(lib, 1), make_ctx(lib, 2)
    lights = torch.zeros(112 * n, dtype=torch.uint8)
    prepared = PreparedLights(own, lights, n) if with_prepared else None
    fp = ForwardPlus(own, w, h, n, prepared=prepared)
    fp.shade_from_tile_lists, fp.use_tile_order = tile_lists, True
    depth, surface = torch.zeros(h, w), torch.zeros(3, h, w, 4)
    ibl = _lib.IblDesc() if with_ibl else None
    lib.take()
    for ctx in (None, other):
        fp.cull(f.cam.frame, lights, n, depth, ctx=ctx)
        radiance = fp.shade(f.cam.frame, surface, lights, n, ibl=ibl, ctx=ctx)
        assert fp.ctx is own and radiance is fp.radiance
        cull, shade = lib.take()
        want = other.handle if ctx is not None else own.handle
        assert (cull[0], cull[1]) == ("sailor_hip_light_cull_prepared", want)
        assert (shade[0], shade[1]) == ("sailor_hip_shade_tile_lists" if tile_lists else "sailor_hip_shade_prepared", want)
        tail = (prepared.buffer.data_ptr(), prepared.capacity) if with_prepared else (None, 0)
        assert cull[2][10] == _lib.CULL_DEFAULT and cull[2][11:] == tail
        a = shade[2]
        assert a[2] == h * w and a[4] == n and a[5:7] == ((TILE_NUM, TILE_LISTS) if tile_lists else (fp.grid.data_ptr(), fp.culled.data_ptr()))
        assert a[7] is None and (a[8] is not None) == with_ibl and a[9] == radiance.data_ptr() and a[11] == TILE_ORDER and a[12:] == tail


def test_shade_before_the_first_cull_reads_the_canonical_lists_in_raster_order(lib):
    fp = ForwardPlus(make_ctx(lib), W, H, 4)
    lib.take()
    fp.shade(_lib.UboFrameData(), torch.zeros(3, H, W, 4), torch.zeros(112 * 4, dtype=torch.uint8), 4)
    (shade,) = lib.take()
    assert shade[0] == "sailor_hip_shade_prepared" and shade[2][5:7] == (fp.grid.data_ptr(), fp.culled.data_ptr())
    assert shade[2][8] is None and shade[2][11] is None and shade[2][12:] == (None, 0)


# ---- EcsSweep ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank,world,trace,want", [(0, 1, "flat", (0, 130)), (1, 2, "flat", (128, 130)), (0, 1, "octree", (0, 130))])
def test_ecs_sweep(lib, rank, world, trace, want):
    ents = synth.make_entities(130)
    sweep = EcsSweep(make_ctx(lib), ents, rank=rank, world=world, trace=trace)
    sweep.run(np.zeros((6, 4), np.float32))
    (call,) = lib.take()
    assert call[0] == "sailor_hip_ecs_sweep_traced" and call[2][0] == 130 and call[2][10:12] == want
    if trace == "flat":
        assert call[2][12] is None
    else:
        assert call[2][12]._obj.mode == _lib.TRACE_OCTREE_INT_BOXES and call[2][12]._obj.dInserted == sweep.inserted.data_ptr()
