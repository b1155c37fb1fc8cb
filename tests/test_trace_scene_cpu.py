"""Row E4 as the reference runs it, without a device: the C-ABI of the octree mode (symbols, constants, the SailorSceneTrace layout), the Python
wrappers' refusal of unknown modes, and the per-entity rule that the kernels implement (include/sailor_hip.h, SAILOR_TRACE_OCTREE_INT_BOXES) held
against the literal octree of oracle.trace_scene_octree_boxes on the edge cases the GPU tests use."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import trace_scene_cases as tc
from oracle import oracle
from sailor_amd import _lib, synth

HEADER = Path(__file__).resolve().parents[1] / "include" / "sailor_hip.h"


def test_the_library_exports_the_traced_entry_points():
    lib = _lib.load()
    for name in ("sailor_hip_ecs_sweep_traced", "sailor_hip_csm_caster_masks_traced"):
        assert getattr(lib, name) is not None
        assert re.search(rf"SAILOR_HIP_API int {name}\(", HEADER.read_text()), name
    assert lib.sailor_hip_version() >= 2


def test_header_constants_are_the_references():
    text = HEADER.read_text()
    define = lambda name: int(re.search(rf"#define {name} (\d+)u", text).group(1))
    assert define("SAILOR_OCTREE_ROOT_SIZE") == oracle.OCTREE_ROOT_SIZE == _lib.OCTREE_ROOT_SIZE == 16536 * 16
    assert define("SAILOR_TRACE_FLAT_FLOAT_BOXES") == _lib.TRACE_FLAT_FLOAT_BOXES == 0
    assert define("SAILOR_TRACE_OCTREE_INT_BOXES") == _lib.TRACE_OCTREE_INT_BOXES == 1


def test_the_ctypes_struct_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "sailor_hip.h"\n'
                   "int main(void) { printf(\"%zu %zu %zu %zu\\n\", sizeof(SailorSceneTrace), offsetof(SailorSceneTrace, mode), "
                   "offsetof(SailorSceneTrace, rootSize), offsetof(SailorSceneTrace, dInserted)); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", str(HEADER.parent), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.SceneTrace
    assert got == [C.sizeof(S), S.mode.offset, S.rootSize.offset, S.dInserted.offset]


def test_the_wrappers_refuse_unknown_modes():
    from sailor_amd.forward_plus import EcsSweep, csm_caster_masks
    ents = synth.make_entities(64)
    for bad in ("bvh", "Octree", "", None):
        with pytest.raises(ValueError):
            _lib.trace_mode(bad)
        with pytest.raises(ValueError):
            EcsSweep(None, ents, trace=bad)
        with pytest.raises(ValueError):
            csm_caster_masks(None, torch.zeros((64, 6)), np.zeros((1, 24), np.float32), trace=bad)
    with pytest.raises(ValueError):   # a root size or inserted words say octree; flat has neither
        EcsSweep(None, ents, trace="flat", octree_root_size=64)
    boxes, planes = torch.zeros((1000, 6)), np.zeros((1, 24), np.float32)
    for short in (torch.zeros(15, dtype=torch.int64), torch.zeros(16, dtype=torch.int32), torch.zeros(32, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError):   # inserted words the kernel would write past, or in the wrong type
            csm_caster_masks(None, boxes, planes, trace="octree", inserted=short)
    assert _lib.trace_mode("flat") == 0 and _lib.trace_mode("octree") == 1


def _rule_is_the_octree(aabb, planes, root):
    """-> (visible, inserted, defined, entities with a negative extent the walk hides and the rule does not)"""
    vis, ins, defined = tc.trace_rule(aabb, planes, root)
    ov, oi, _, _ = oracle.trace_scene_octree_boxes(tc.oracle_safe(aabb, tc.oracle_comparable(aabb), root), planes, root_size=root)
    n = len(aabb)
    hidden = tc.check_against_the_walk(vis, ins, tc.bits(ov, n), tc.bits(oi, n), aabb)
    return vis, ins, defined, hidden


def test_the_per_entity_rule_is_the_octree_walk_on_the_edge_cases():
    """truncation towards zero, extents below one, inverted boxes, both directions of disagreement with the float test, centres above 2^24 under a
    root of 2^30, integer faces on +-h and one unit inside.  Boxes with a negative truncated extent: the stated divergence -- the walk's visible set
    is a proper subset of the rule's there (it depends on where the other elements put the element), the inserted bits are equal."""
    aabb, planes, root = tc.truncation_case()
    assert tc.negative_extent(aabb).sum() > 1000
    float_only = octree_only = hidden = 0
    for k in range(len(planes)):
        vis, ins, _, h = _rule_is_the_octree(aabb, planes[k], root)
        assert ins.all()
        exact = tc.walk_exact(aabb)
        flat = tc.overlaps(planes[k], aabb[:, :3], aabb[:, 3:])
        float_only += int((flat & ~vis)[exact].sum()); octree_only += int((vis & ~flat)[exact].sum()); hidden += h
    assert float_only > 0 and octree_only > 0 and hidden > 0
    aabb, planes, root = tc.large_case()
    for k in range(len(planes)):
        assert _rule_is_the_octree(aabb, planes[k], root)[3] == 0
    for r in (64, 1000):
        faces, root = tc.root_faces_case(r)
        vis, ins, _, _ = _rule_is_the_octree(faces, tc.one_plane((0, 0, 0), 1.0), root)
        assert 0 < ins.sum() < len(faces) and np.array_equal(vis, ins)


def test_undefined_boxes_are_neither_inserted_nor_visible_by_the_rule():
    aabb, planes, root = tc.truncation_case()
    mixed = tc.with_undefined(aabb)
    vis, ins, defined, _ = _rule_is_the_octree(mixed, planes[3], root)
    assert (~defined).sum() == len(tc.UNDEFINED)
    assert not vis[~defined].any() and not ins[~defined].any()
