"""CPU suite of the ShadowPrepass and Clear nodes: the new symbols and the opt-in, and the runtime's pass planning (LightingECS::PlanLightPasses /
CountBatchRuns through sailor_rt_csm_planner_*, no device) held against tests/shadow_prepass_ref.py, a Python restatement of ECS/LightingECS.cpp:262-371 built on
host.plan_csm_passes.  The overlap sets are written down by hand, not computed: 200 instances, three batches."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import shadow_prepass_ref as ref
from sailor_amd import _lib, host, runtime_binding
from shadow_prepass_ref import EVSM, PCF, mask_of

ROOT = Path(__file__).resolve().parents[1]
N = 200
BATCHES = [(0, 64), (64, 1), (65, 135)]     # (firstInstance, instanceCount): a word, one instance, the rest
IDENTITY = (0.0, 0.0, 0.0, 1.0)
HIP_SYMBOLS = ("sailor_hip_shadow_gather_instances", "sailor_hip_shadow_gather_instances_batched", "sailor_hip_shadow_gather_workspace_bytes",
               "sailor_hip_shadow_extract_positions", "sailor_hip_buffer_fill_pattern")
RT_SYMBOLS = ("sailor_rt_set_caster_data", "sailor_rt_set_light_rotation", "sailor_rt_shadow_passes", "sailor_rt_csm_shadow_map", "sailor_rt_lights_matrices",
              "sailor_rt_csm_planner_create", "sailor_rt_csm_planner_destroy", "sailor_rt_csm_planner_frame")


def view(camera=(0.0, 0.0, 0.0), light=0):
    return (light, (*camera, 1.0), IDENTITY, (0.0, 100.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5))


def sets(shared=()):
    """one light's four overlap sets: cascade k overlaps its own band of instances (the bands are disjoint), plus the instances listed in `shared` as
    (instance, cascade, cascade): a caster that two cascades overlap"""
    bands = [set(range(0, 40)), set(range(50, 90)), set(range(100, 150)), set(range(160, 200))]
    for instance, a, b in shared:
        bands[a].add(instance)
        bands[b].add(instance)
    return np.stack([mask_of(sorted(b), N) for b in bands])


def ids(p):
    return ref.bits(p["mask"], N).nonzero()[0].tolist()


class Both:
    """the runtime's planner and the restatement, fed the same frames"""

    def __init__(self):
        self.native, self.ref = runtime_binding.CsmPlanner(), ref.Planner()

    def frame(self, light_types, views, overlap, frames, cast=None, batches=BATCHES):
        got = self.native.frame(light_types, [host._csm_view_struct(v) for v in views], N, overlap, frames, cast, batches)
        want = self.ref.frame(light_types, views, N, overlap, frames, cast, batches)
        assert len(got) == len(want), (got, want)
        for g, w in zip(got, want):
            assert (g["light"], g["cascade"], g["shadow_type"], g["casters"], g["dependencies"]) == (w["light"], w["cascade"], w["shadow_type"], w["casters"], w["dependencies"]), (g, w)
            np.testing.assert_array_equal(g["mask"], w["mask"])
            np.testing.assert_array_equal(g["runs"], w["runs"])
        return got

    def close(self):
        self.native.close()


@pytest.fixture
def both():
    b = Both()
    yield b
    b.close()


def test_symbols_and_opt_in():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    declared = set(re.findall(r"\b(sailor_(?:hip|host)_\w+)\s*\(", header))
    lib, rt = _lib.load(), runtime_binding.load()
    for name in HIP_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in RT_SYMBOLS:
        assert hasattr(rt, name), name
    assert C.sizeof(_lib.ShadowGatherJob) == 40 and lib.sailor_hip_version() >= 10
    assert rt.sailor_rt_enable_node(None, b"ShadowPrepass") == -1 and rt.sailor_rt_enable_node(None, b"Clear") == -1   # no runtime: nothing to opt in
    assert rt.sailor_rt_node_registered(b"ShadowPrepass") == 0 and rt.sailor_rt_node_registered(b"Clear") == 0            # opt-in classes stay unregistered
    # the workspace is a function of the ranges alone: 4 bytes per 1 024 bits, rounded up to 256
    jobs = (_lib.ShadowGatherJob * 3)(_lib.ShadowGatherJob(None, 0, 1024, None, 0, 0, None), _lib.ShadowGatherJob(None, 5, 5, None, 0, 0, None),
                                      _lib.ShadowGatherJob(None, 7, 7 + 64 * 1024 + 1, None, 0, 0, None))
    assert lib.sailor_hip_shadow_gather_workspace_bytes(jobs, 3) == 512 and lib.sailor_hip_shadow_gather_workspace_bytes(jobs, 2) == 256
    assert lib.sailor_hip_shadow_gather_workspace_bytes(None, 0) == 0


@pytest.mark.parametrize("light_type", [PCF, EVSM])
def test_first_frame_four_passes_second_identical_frame_none(both, light_type):
    frames = np.zeros(N, np.uint64)
    passes = both.frame([light_type], [view()], sets(), frames)
    assert [p["cascade"] for p in passes] == [0, 1, 2, 3]
    assert [p["shadow_type"] for p in passes] == [light_type, PCF, PCF, PCF]
    assert [p["dependencies"] for p in passes] == [[], [], [], []]
    assert both.frame([light_type], [view()], sets(), frames) == []


def test_camera_moved_below_and_above_the_threshold(both):
    frames = np.zeros(N, np.uint64)
    assert len(both.frame([PCF], [view()], sets(), frames)) == 4
    assert both.frame([PCF], [view((14.9, 0.0, 0.0))], sets(), frames) == []
    # a kept snapshot keeps its camera (:353-357): 15.1 from where the snapshots were TAKEN re-renders every cascade
    assert [p["cascade"] for p in both.frame([PCF], [view((15.1, 0.0, 0.0))], sets(), frames)] == [0, 1, 2, 3]
    assert both.frame([PCF], [view((15.1, 0.0, 14.0))], sets(), frames) == []


def test_one_instance_changed_only_the_cascades_whose_final_set_holds_it(both):
    frames = np.zeros(N, np.uint64)
    both.frame([PCF], [view()], sets(), frames)
    frames[60] = 7
    passes = both.frame([PCF], [view()], sets(), frames)
    assert [p["cascade"] for p in passes] == [1] and 60 in ids(passes[0])
    frames[45] = 9   # in no cascade's set
    assert both.frame([PCF], [view()], sets(), frames) == []
    frames[10], frames[170] = 11, 11
    assert [p["cascade"] for p in both.frame([PCF], [view()], sets(), frames)] == [0, 3]


def test_a_caster_in_cascades_1_and_2_is_removed_from_2_which_depends_on_pass_1(both):
    frames = np.zeros(N, np.uint64)
    overlap = sets([(95, 1, 2)])
    by = {p["cascade"]: p for p in both.frame([PCF], [view()], overlap, frames)}
    assert 95 in ids(by[1]) and 95 not in ids(by[2])
    assert ids(by[2]) == list(range(100, 150))
    assert by[0]["dependencies"] == [] and by[1]["dependencies"] == [] and by[2]["dependencies"] == [1] and by[3]["dependencies"] == []
    assert sum(r[0] for r in by[2]["runs"].tolist()) == 50


def test_the_same_caster_with_cascade_1_unchanged_is_not_removed_and_there_is_no_dependency(both):
    """The reference's own second frame over that scene: nothing has changed, cascade 1's snapshot is equal and it is NOT re-rendered, so bCascadeAdded[1] is
    None, cascade 2 keeps the caster it shares with cascade 1 (:315-318) -- which makes its list differ from its snapshot, and it is drawn again, alone and
    without a dependency.  The third frame is quiet."""
    frames = np.zeros(N, np.uint64)
    overlap = sets([(95, 1, 2)])
    both.frame([PCF], [view()], overlap, frames)
    passes = both.frame([PCF], [view()], overlap, frames)
    assert [p["cascade"] for p in passes] == [2]
    assert passes[0]["dependencies"] == [] and 95 in ids(passes[0]) and ids(passes[0]) == [95] + list(range(100, 150))
    assert both.frame([PCF], [view()], overlap, frames) == []


def test_the_shift_arithmetic_when_an_earlier_cascade_was_not_re_rendered(both):
    """`alreadyPlacedPasses + shift` (:307-331) counts only the cascades that were added this frame: with cascades 0 and 1 unchanged, cascade 2 is pass 0 of the
    frame and cascade 3, which loses the caster it shares with it, lists 0"""
    frames = np.zeros(N, np.uint64)
    overlap = sets([(95, 1, 2), (155, 2, 3)])
    first = {p["cascade"]: p["dependencies"] for p in both.frame([PCF], [view()], overlap, frames)}
    assert first == {0: [], 1: [], 2: [1], 3: [2]}
    for _ in range(4):   # the scene settles: each cascade in turn takes back what the one before it no longer removes
        both.frame([PCF], [view()], overlap, frames)
    assert both.frame([PCF], [view()], overlap, frames) == []
    frames[120] = 5      # cascade 2's own
    passes = both.frame([PCF], [view()], overlap, frames)
    assert [p["cascade"] for p in passes] == [2, 3]
    assert passes[0]["dependencies"] == [] and 95 in ids(passes[0])   # cascade 1 was not added: nothing removed from cascade 2
    assert passes[1]["dependencies"] == [0] and 155 not in ids(passes[1])


def test_an_evsm_light_never_makes_cascade_0_a_dependency_source(both):
    frames = np.zeros(N, np.uint64)
    overlap = sets([(45, 0, 1), (46, 0, 2), (95, 1, 2)])
    by = {p["cascade"]: p for p in both.frame([EVSM], [view()], overlap, frames)}
    assert by[0]["shadow_type"] == EVSM
    assert 45 in ids(by[0]) and 45 in ids(by[1]) and 46 in ids(by[2])   # shared with cascade 0 and kept: another shadow type (:315-318)
    assert by[1]["dependencies"] == [] and by[2]["dependencies"] == [1] and by[3]["dependencies"] == []
    # the same sets under a PCF light: cascade 0 removes, and is a dependency of both
    native, restated = runtime_binding.CsmPlanner(), ref.Planner()
    try:
        pcf = native.frame([PCF], [host._csm_view_struct(view())], N, overlap, frames, None, BATCHES)
    finally:
        native.close()
    assert [p["dependencies"] for p in pcf] == [p["dependencies"] for p in restated.frame([PCF], [view()], N, overlap, frames, None, BATCHES)] == [[], [0], [0, 1], []]


def test_two_lights_and_the_snapshot_count_rule(both):
    frames = np.zeros(N, np.uint64)
    two = np.stack([sets([(95, 1, 2)]), sets([(95, 1, 2)])])
    passes = both.frame([EVSM, PCF], [view(light=0), view(light=1)], two, frames)
    assert [(p["light"], p["cascade"]) for p in passes] == [(l, k) for l in range(2) for k in range(4)]
    assert passes[2]["dependencies"] == [1] and passes[6]["dependencies"] == [5]   # alreadyPlacedPasses = 4 for the second light
    both.frame([EVSM, PCF], [view(light=0), view(light=1)], two, frames)
    assert both.frame([EVSM, PCF], [view(light=0), view(light=1)], two, frames) == []
    # one light fewer: the snapshots no longer fit the view and are dropped (:391-397), everything is rendered again
    assert len(both.frame([EVSM], [view(light=0)], two[:1], frames)) == 4


def test_cast_shadows_is_anded_in_after_the_planning_and_the_runs_are_popcounts(both):
    frames = np.zeros(N, np.uint64)
    rng = np.random.default_rng(3)
    cast = ref.words_of(rng.random(N) < 0.6)
    cast_bits = ref.bits(cast, N)
    cast_bits[95] = False
    cast = ref.words_of(cast_bits)
    passes = both.frame([PCF], [view()], sets([(95, 1, 2)]), frames, cast)
    for p in passes:
        b = ref.bits(p["mask"], N)
        assert not (b & ~cast_bits).any()
        for (first, count), (run_count, run_offset) in zip(BATCHES, p["runs"].tolist()):
            assert run_count == int(b[first:first + count].sum())
            assert run_offset == int(b[:first].sum())   # the batches tile the instances in order here
        assert p["casters"] == int(b.sum())
    # the dependencies do not look at m_bCastShadows: they are decided on the proxies' lists (:321-330), the node filters afterwards (ShadowPrepassNode.cpp:110)
    assert [p["dependencies"] for p in passes] == [[], [], [1], []]
    # batches that leave instances out: the runs count what the batches hold
    some = both.frame([PCF], [view((100.0, 0.0, 0.0))], sets(), frames, None, [(10, 20), (170, 5)])
    assert [p["runs"].tolist() for p in some] == [[[20, 0], [0, 20]], [[0, 0], [0, 0]], [[0, 0], [0, 0]], [[0, 0], [5, 0]]]


def test_the_runtime_tests_scene_keeps_every_caster_in_one_cascade():
    """tests/shadow_prepass_cases.py says why: the CPU oracle's overlap sets of the layout, for the camera of the test and for the camera moved by 16 units;
    the shared box of the second layout lies in cascades 1 and 2; and every cascade's casters leave fragments in its map (oracle.raster_depth)"""
    import shadow_prepass_cases as sc
    from oracle import oracle
    for shared in (False, True):
        L = sc.layout(shared)
        for position in ((0.0, 150.0, 0.0), (16.0, 150.0, 0.0)):
            cam = sc.camera(position)
            masks = oracle.csm_caster_masks(L.world_aabb, sc.cascade_planes(cam))
            inside = np.stack([ref.bits(masks[k], L.num_instances) for k in range(4)])
            for i, slab in enumerate(L.slab_of):
                want = [False] * 4
                if slab >= 0:
                    want[slab] = True
                if slab == -2:
                    want[1] = want[2] = True
                assert inside[:, i].tolist() == want, (shared, position, i, slab, inside[:, i])
    L, cam = sc.layout(False), sc.camera()
    lm = sc.lights_matrices(cam)
    for k in range(4):
        own = np.uint32([i for i, slab in enumerate(L.slab_of) if slab == k])
        depth = np.zeros((64, 64), np.float32)
        for count, n, first_index, vertex_offset, first_instance in L.batches.tolist():
            ids = own[(own >= first_instance) & (own < first_instance + n)]
            depth = oracle.raster_depth(lm[k], L.vertices[vertex_offset:, 2:5], L.indices[first_index:first_index + count], L.instances["model"], 64, 64,
                                        instance_ids=ids, depth=depth, cull_back=True)
        assert (depth > 0).mean() > 0.2 and depth.max() <= 1.0, k
