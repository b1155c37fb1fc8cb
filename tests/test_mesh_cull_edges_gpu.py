"""The instance visibility kernels (k4_mesh_frustum_cull<false / true>, msc_occluded, hiz_fetch_min, k_hiz_downscale, k_hiz_tail, k4_draw_*) on the
placed cases of tests/mesh_cull_cases.py: every word of every record, the indirect buffer and the pyramids equal the C oracle's, and the float64
reference's wherever that is decided.  tests/test_mesh_cull_cpu.py holds the same cases against each other on the CPU (and the mutant table)."""
import numpy as np
import pytest
import torch

import mesh_cull_cases as cases
from oracle import oracle, oracle_f64
from sailor_amd.forward_plus import MeshCull, hiz_build

pytestmark = pytest.mark.gpu

NO_BATCHES = np.zeros((0, 5), np.uint32)


def _words(records: np.ndarray) -> np.ndarray:
    return records.view(np.uint32).reshape(-1, 24)


def _hiz_arg(ctx, hiz):
    return None if hiz is None else (torch.from_numpy(hiz[0]).to(ctx.device),) + tuple(hiz[1:])


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_flags_equal_the_oracle_and_the_decided_reference(ctx, name):
    """flags only (numBatches = 0): the 24 words of every record are the input's with word 21 = the C oracle's flag; where the float64 reference is
    decided the flag is the reference's too.  scene-* cases also go through the compact entry point as one draw.

    Measured on an MI355X: the unmodified kernels pass every test of this file (55, about 4 s).  Compare-only mutants of the kernel library (scratch
    copies, in-bounds changes) and the tests of this file that fail on them:
      depthSphere <= depth     this test [exact-depth-tie]
      Cz <= r + znear          this test [exact-gate, footprint-16x16, footprint-24x10], test_footprints_under_the_one_texel_probe [both]
      dot <= -radius           this test [flip-plane-tie-zero-radius, flip-planes-identity, flip-planes-camera]
      cz - radius >= zFar      this test [exact-zrange]
      useX1 always true        test_footprints_under_the_one_texel_probe [footprint-24x10], test_hiz_shapes_equal_the_oracle_and_the_reference [11 shapes]"""
    case, ref = cases.build(name), cases.reference(name)
    hiz = _hiz_arg(ctx, case.hiz)
    mc = MeshCull(ctx, case.instances, NO_BATCHES)
    mc.run(case.frame, hiz=hiz)
    got, _ = mc.download()
    want = _words(case.instances).copy()
    want[:, 21] = cases.oracle_flags(name)
    np.testing.assert_array_equal(_words(got), want)
    dec = ref["decided"]
    np.testing.assert_array_equal(got["isCulled"][dec] == 1, ref["culled"][dec])
    if name.startswith("scene-"):
        batches = cases.batches_of([0], [len(case.instances)])
        mc = MeshCull(ctx, case.instances, batches)
        mc.run(case.frame, hiz=hiz)
        got_i, got_b = mc.download()
        ref_i, ref_b = oracle.mesh_cull_compact(case.frame, case.instances, len(case.instances), 0, batches, hiz=case.hiz)
        np.testing.assert_array_equal(got_b, ref_b)
        np.testing.assert_array_equal(_words(got_i), _words(ref_i))
        assert 0 < got_b[0, 1] < len(case.instances)


@pytest.mark.parametrize("name", cases.PROBE_NAMES)
def test_footprints_under_the_one_texel_probe(ctx, name):
    """one MeshCull, one pyramid tensor, one texel rewritten per probe (341 / 316 launches of a 33-instance cull): the probes an instance survives
    are the C oracle's always and the float64 footprint where frustum, gate, level and both axes are decided"""
    case, ref = cases.build(name), cases.reference(name)
    pyr, W, H, levels = _hiz_arg(ctx, case.hiz)
    mc = MeshCull(ctx, case.instances, NO_BATCHES)
    flag = mc.instances.view(torch.int32).view(-1, 24)[:, 21]
    out = torch.empty((pyr.numel(), len(case.instances)), dtype=torch.int32, device=ctx.device)
    for t in range(pyr.numel()):
        pyr[t] = float(cases.PROBE_HOLE)
        mc.run(case.frame, hiz=(pyr, W, H, levels))
        out[t].copy_(flag)
        pyr[t] = float(cases.PROBE_FILL)
    ctx.synchronize()
    got = out.cpu().numpy() == 0
    np.testing.assert_array_equal(got, cases.oracle_probe_survivors(name))
    dec = ref["frustum_decided"] & ref["gate_decided"] & ref["level_decided"] & ref["footprint_decided"]
    np.testing.assert_array_equal(got[:, dec], cases.reference_probe_survivors(name)[:, dec])
    for i, k in case.texels.items():
        assert got[:, i].sum() == k
    after, _ = mc.download()
    keep = np.ones(24, bool); keep[21] = False
    np.testing.assert_array_equal(_words(after)[:, keep], _words(case.instances)[:, keep])


@pytest.mark.parametrize("name", cases.HIZ_NAMES)
def test_hiz_shapes_equal_the_oracle_and_the_reference(ctx, name):
    """sailor_hip_hiz_build on every shape of cases.HIZ_SHAPES (k_hiz_downscale and both sides of k_hiz_tail's entry condition): bit for bit the C
    oracle's, a texel that is NaN by class; and the float64 downscale of its own level below wherever the footprints agree"""
    raw, W, H, levels, _ = cases.hiz_source(name)
    got = hiz_build(ctx, torch.from_numpy(raw).to(ctx.device), W, H, levels).cpu().numpy()
    want = cases.hiz_oracle(name)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    ref = oracle_f64.hiz_build(raw, W, H, levels, given=got)
    clean = ref["agree"] & ~ref["nan"]
    np.testing.assert_array_equal(got[clean].astype(np.float64), ref["pyramid"][clean])


# ---- compaction --------------------------------------------------------------------------------------------------------------------------------
def _run_compaction(ctx, inst, batches, mc=None):
    cam = cases.compact_camera()
    if mc is None:
        mc = MeshCull(ctx, inst, batches)
    mc.run(cam.frame)
    got_i, got_b = mc.download()
    want_words, want_batches = cases.compact_expected(cam.frame, inst, batches)     # the C oracle's flags, the NumPy partition
    np.testing.assert_array_equal(got_b, want_batches)
    np.testing.assert_array_equal(_words(got_i), want_words)
    ref_i, ref_b = oracle.mesh_cull_compact(cam.frame, inst, len(inst), 0, batches)  # and the C oracle's own step 3
    np.testing.assert_array_equal(got_b, ref_b)
    np.testing.assert_array_equal(_words(got_i), _words(ref_i))
    return got_i, got_b


@pytest.mark.parametrize("count", cases.COMPACT_COUNTS)
def test_compaction_at_chunk_and_look_back_sizes(ctx, count):
    """one draw of 0 / 1 / 255 .. 513 records (the 256-record chunk), 64 * 256 and 64 * 256 + 1 (a look-back of exactly 64 predecessors) and
    65 * 256 + 1 (65: a second look-back step), under every keep pattern"""
    for pattern in cases.COMPACT_PATTERNS:
        inst, batches = cases.compact_single(count, pattern)
        _, got_b = _run_compaction(ctx, inst, batches)
        assert got_b[0, 1] == cases.keep_pattern(pattern, count).sum(), pattern


@pytest.mark.parametrize("num_batches", cases.COMPACT_BATCH_NUMBERS)
def test_compaction_at_the_plans_scan_width(ctx, num_batches):
    """1023 / 1024 / 1025 / 2049 draws: the 1024-wide scan of k4_draw_plan and its carry"""
    inst, batches = cases.compact_many(num_batches)
    _run_compaction(ctx, inst, batches)


def test_compaction_with_gaps_and_unordered_draws(ctx):
    inst, batches = cases.compact_gaps()
    got_i, _ = _run_compaction(ctx, inst, batches)
    owned = np.zeros(len(inst), bool)
    for f, c in zip(batches[:, 4], batches[:, 1]):
        owned[f:f + c] = True
    keep = np.ones(24, bool); keep[21] = False
    np.testing.assert_array_equal(_words(got_i)[~owned][:, keep], _words(inst)[~owned][:, keep])


def test_one_workspace_for_two_differently_shaped_calls(ctx):
    """a 66-chunk single draw, then three short draws through the SAME workspace bytes: nothing of the first plan (item list, status words, tickets)
    may leak into the second"""
    big_i, big_b = cases.compact_single(65 * 256 + 1, "alternating")
    big = MeshCull(ctx, big_i, big_b)
    _run_compaction(ctx, big_i, big_b, big)
    keep = (np.arange(700) * 3) % 5 < 2
    small_i, small_b = cases.compact_records(keep), cases.batches_of([0, 300, 301], [300, 1, 399])
    small = MeshCull(ctx, small_i, small_b)
    assert small._ws_bytes <= big._ws_bytes
    small.workspace = big.workspace
    _run_compaction(ctx, small_i, small_b, small)
    _run_compaction(ctx, big_i, big_b, MeshCull(ctx, big_i, big_b))
