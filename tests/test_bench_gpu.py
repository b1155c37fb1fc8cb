"""bench.py's output contract on a real device: a plain run's headline line and its --dump-outputs; with --full, one JSON line with the driver's
keys, the `roofline` and `cpu_baseline` objects, and -- with a one-rank RCCL process group -- both multi-GPU modes (the split frame + list
exchange as `value`, a frame per GPU next to it; `--frame-per-gpu` swaps them)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _run(cmd, env=None):
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    if p.returncode != 0:   # (the first lines that are not stack frames say what happened; the tail alone is a C++ back trace)
        head = [l for l in p.stderr.splitlines() if "frame #" not in l][:40]
        raise AssertionError(f"rc {p.returncode}\n" + "\n".join(head) + "\n...\n" + p.stderr[-1500:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "rank 0 prints ONE JSON line"
    # ... and nothing else reaches stdout: what RCCL / Gloo / the other ranks print through C stdio is on stderr (bench.claim_stdout)
    assert p.stdout.strip() == lines[0], p.stdout[:400]
    return json.loads(lines[0])


def test_default_line_carries_the_contract():
    d = _run([sys.executable, "bench.py", "--full", "--steps", "5", "--warmup", "2", "--spinup-ms", "50", "--cpu-sample-tile-rows", "4"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in d, key
    assert d["unit"] == "Mpixels/s" and d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert "3 steps of the frame pipeline per graph, 2 in the last" in d["launch"] and "3 list sets" in d["launch"]   # K not a multiple of the list sets: exactly K steps all the same
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic" and d["scaling"] in ("weak", "strong")
    assert d["config"]["workload"].startswith("C3: 3840x2160, 65536 ") and "model" not in d["config"]
    assert abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["kernel"] == "k2_shade_pt"   # prepared lights, lists from the cull's per-tile slots: the default path
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.05 < r["frac"] < 1.0
    assert abs(r["achieved"] - r["bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] > 0.9 * r["bytes_per_launch"]
    # round 4: the roofline's duration is a DIRECT reading of the kernel -- an event pair around every launch, each launch between its real neighbours --
    # not a difference of two medians; the difference and the back-to-back figure ride along as secondary fields
    st = r["avg_launch_ms_stats"]
    assert st["launches"] >= 50 and st["min"] <= st["median"] <= st["max"] and abs(r["avg_launch_ms"] - st["mean"]) < 1e-12 and "event pair on the dispatch packet of EVERY launch" in r["timing"]
    assert abs(r["in_frame_by_difference_ms"] - (d["serial_step_ms"]["median"] - d["cull_ms"])) < 1e-9
    # sanity between the readings of the same kernel (no gate on a committed artefact: rocprof_kernel_avg_ms is informational and may be stale or None)
    assert 0.8 * r["back_to_back_launch_ms"] < r["avg_launch_ms"] < 1.25 * r["back_to_back_launch_ms"]
    assert r["in_frame_by_difference_ms"] < r["avg_launch_ms"] * 1.10
    assert r["rocprof_kernel_avg_ms"] is None or r["rocprof_kernel_avg_ms"] > 0
    assert 0.05 < r["whole_path"]["frac_serial"] < 1.0 and 0.05 < r["whole_path"]["frac_pipelined"] < 1.0
    # both light modes in the line; C3 is quoted with static lights
    assert d["lights"]["mode"].startswith("static") and d["lights"]["prepare_lights_ms"] > 0
    assert d["ms_per_step_dynamic"] > d["ms_per_step"] * 0.8 and d["value_dynamic_lights"] > 0   # (five steps: the two readings are within noise of each other since the preparation rides in the cull)
    assert d["value_serial"] > 0 and d["serial_step_ms"]["min"] <= d["serial_step_ms"]["median"] <= d["serial_step_ms"]["max"]
    assert abs(d["value_serial"] - 3840 * 2160 / (d["serial_step_ms"]["median"] * 1e-3) / 1e6) < 1e-6 * d["value_serial"]
    assert d["value_serial"] < d["value"] * 1.10, "one frame in flight is not faster than two (five steps: a loose bound)"
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["unit"] == "Mpixels/s" and c["value"] > 0 and "tile rows" in c["sample"]
    for block in ("ecs_sweep", "mesh_cull_compact", "linearize_depth", "ambient_ibl", "evsm_blur", "ibl_prefilter", "shadow_passes"):
        assert block in d, block
    # round 6: the shadow passes one by one (the figure of record) and side by side on four streams -- the same depth buffers, bit for bit
    sp = d["shadow_passes"]
    assert sp["all_passes_ms"] > 0 and sp["side_by_side_equals_one_by_one"] is True and 0 < sp["all_passes_side_by_side_ms"] <= sp["all_passes_ms"] * 1.1
    # round 5: the box's own yardstick (a float4 copy timed in this process) beside the guide's constant, the chain's kernels as the library names them,
    # when k1_pack runs, and K4's slices of a 2- / 4- / 8-way entity split timed on this one GPU
    assert 2000.0 < d["box"]["copy_gbs"] < 8000.0 and abs(r["frac_of_box_copy"] - r["achieved"] / d["box"]["copy_gbs"]) < 1e-9
    assert list(r["cull"]["kernels_ms"]) == ["k01_prepare", "k1_group_lists", "k1_tile_cull", "k1_pack"] and d["pack"]["mode"] == "deferred"
    sim = d["ecs_sweep"]["split"]["split_simulated_on_one_gpu"]
    assert set(sim) == {"2", "4", "8"} and all(v["slice_ms_max"] > 0 for v in sim.values()) and d["ecs_sweep"]["split"]["default"] == "replicated"


def test_a_plain_run_prints_the_headline_and_dumps_the_last_steps_outputs(tmp_path):
    """Without --full: the headline alone (no further reading), and --dump-outputs writes what the last timed step computed -- the frame's lists bit
    for bit and its radiance within 1e-4 relative of the oracle, as smoke() holds them."""
    import numpy as np

    from oracle import oracle
    from sailor_amd import synth
    d = _run([sys.executable, "bench.py", "--config", "tiny", "--steps", "7", "--warmup", "2", "--spinup-ms", "50", "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 7 and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert abs(d["value"] - 128 * 96 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    assert [k for k in ("step_ms", "roofline", "box", "serial_step_ms", "value_dynamic_lights", "cpu_baseline", "ecs_sweep") if k in d] == []
    f = synth.make_frame("tiny")
    og, oi, _ = oracle.light_cull(f.cam.frame, 128, 96, f.lights, f.depth)
    orad = oracle.shade(f.cam.frame, 128, 96, f.surface, f.lights, og, oi, None)
    np.testing.assert_array_equal(np.load(tmp_path / "light_grid.npy"), og.astype(np.float64))
    np.testing.assert_array_equal(np.load(tmp_path / "culled_lights.npy"), oi[: 1 + int(oi[0])].astype(np.float64))
    rad = np.load(tmp_path / "radiance.npy")
    assert rad.dtype == np.float32 and rad.shape == (96, 128, 4)
    err = np.abs(rad.astype(np.float64) - orad)
    assert (err <= 1e-4 * np.abs(orad)).all(), f"radiance differs from the oracle: max abs err {err.max()}"


@pytest.mark.parametrize("split_primary", [True, False])
def test_one_rank_process_group_runs_both_multi_gpu_modes(split_primary):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--force-dist", "--full", "--steps", "5", "--warmup", "2", "--spinup-ms", "50", "--no-cpu-baseline"]
    d = _run(cmd + ([] if split_primary else ["--frame-per-gpu"]), env)
    assert d["scaling"] == ("strong" if split_primary else "weak")  # the default headline is the split frame (BASELINE.json's metric)
    other = d["alternate_frame_rendering"] if split_primary else d["split_frame"]
    assert other["scaling"] == ("weak" if split_primary else "strong") and other["value"] > 0 and "error" not in other
    ex = d["exchange"] if split_primary else d["split_frame"]["exchange"]
    assert ex["tiles"] == 240 * 135 and ex["global_sum_num"] == d["config"]["sum_num_rank0_band"] and ex["checksum"] > 0
    assert "sailor_hip_exchange_light_lists_rows" in ex["how"]   # the shipped exchange (C-ABI over an ncclComm_t), not torch.distributed's collectives
    # round 6: the exchange's own cost is in the line -- event-timed record-only calls, the slots of the second gather sized by sailor_hip_exchange_adapt
    assert ex["timed_exchanges"] >= 10 and 0 < ex["ms_min"] <= ex["ms_median"] <= ex["ms_p90"] and ex["ms_first_worst_case_slots"] > 0
    assert ex["largest_band_total"] == ex["global_sum_num"] and ex["clipped"] is False
    assert ex["slot_words"] == (ex["global_sum_num"] + ex["global_sum_num"] // 4 + 1 + 63) // 64 * 64 < ex["worst_case_slot_words"] == 240 * 135 * 128
    assert ex["bytes_gathered"] == 4 * (1 + ex["slot_words"] + 2 * 240 * 135)
    if split_primary:
        assert d["speedup_vs_one_gpu_whole_frame"] > 0
    assert d["step_ms"]["p10"] <= d["step_ms"]["median"] <= d["step_ms"]["p90"]


@pytest.mark.parametrize("ranks", [2, 3])
def test_ranks_sharing_the_gpu_run_the_split_frame_for_real(ranks):
    """`python bench.py --gpus N` as the driver types it (no launcher: bench.py starts its ranks itself), N > 1, on a ONE-GPU box: with
    SAILOR_BENCH_SHARE_GPU=1 every rank takes device 0 over a `gloo` group.  The figures mean nothing (the ranks time-share the device); the path is the
    real one -- calibration cull, cost-balanced re-split, band kernels inside the pipeline graph, every collective of main(), the list exchange -- and the
    exchanged global lists must be the ones a single rank holds for the whole frame."""
    common = ["--full", "--steps", "6", "--warmup", "2", "--spinup-ms", "50", "--no-cpu-baseline"]
    env1 = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    one = _run([sys.executable, "bench.py", "--gpus", "1", "--force-dist", "--no-afr"] + common, env1)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SAILOR_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    d = _run([sys.executable, "bench.py", "--gpus", str(ranks)] + common, env)
    assert d["n_gpus"] == ranks and d["scaling"] == "strong" and d["steps"] == 6 and f"tile-row bands x{ranks}" == d["config"]["parallelism"]
    bounds = d["exchange"]["tile_row_bounds"]
    assert len(bounds) == ranks + 1 and bounds[0] == 0 and bounds[-1] == 135 and all(a < b for a, b in zip(bounds, bounds[1:])) and "cost-balanced" in d["config"]["partition"]
    assert abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]      # ONE frame per step, whatever the rank count
    for key in ("tiles", "global_sum_num", "checksum"):                                             # the frame's lists, rebuilt from the bands == one rank's whole frame
        assert d["exchange"][key] == one["exchange"][key], key
    assert "torch.distributed (gloo)" in d["exchange"]["how"]                                       # RCCL takes one rank per device: all ranks agreed on the fallback
    # round 6: what the exchange costs is in every N > 1 line: its event-timed duration, the bytes gathered, and the step with the exchange in it
    assert d["exchange"]["timed_exchanges"] >= 10 and 0 < d["exchange"]["ms_median"] <= d["exchange"]["ms_p90"] and d["exchange"]["bytes_gathered"] > 0
    assert 0 < d["value_exchange_every_step"] and d["ms_per_step_exchange_every_step"] > d["ms_per_step_same_form_without_exchange"] * 0.5 > 0
    assert d["alternate_frame_rendering"]["value"] > 0 and "error" not in d["alternate_frame_rendering"]
    # round 5: an N > 1 line of the headline also carries bounded split readings of the two configurations BASELINE.json names for a node, the bands re-cut
    # on measured times, and K4 across the ranks (entity ranges + one all-gather of the visibility words) beside K4 replicated -- the gathered bitmask is
    # the replicated sweep's on every rank
    assert list(d["split_configs"]) == ["C4", "C5"]
    for name, v in d["split_configs"].items():
        assert "error" not in v and v["split_ms_per_step"] > 0 and v["whole_frame_per_gpu_ms_per_step"] > 0 and v["speedup_vs_one_gpu_whole_frame"] > 0, (name, v)
        assert v["tile_row_bounds"][0] == 0 and len(v["tile_row_bounds"]) == ranks + 1
        assert v["exchange"]["ms_median"] > 0 and v["exchange"]["bytes_gathered"] > 0 and 0 < v["value_exchange_every_step"] < v["value"], (name, v.get("exchange"))
    assert d["split_configs"]["C5"]["lights"].startswith("dynamic") and d["split_configs"]["C5"]["tile_row_bounds"][-1] == 270
    e = d["ecs_sweep"]["split"]
    assert e["default"] == "replicated" and e["entities"] == 1 << 20 and e["split"]["ranks"] == ranks and e["split"]["bitmask_equals_replicated_on_every_rank"] is True
    assert e["split"]["slice_ms"] < e["replicated_ms"] * 1.5


@pytest.mark.parametrize("sets, steps", [(3, 12), (2, 8)])
def test_step_counts_the_list_sets_divide_run_one_pipeline_graph(sets, steps):
    d = _run([sys.executable, "bench.py", "--full", "--steps", str(steps), "--warmup", "2", "--spinup-ms", "50", "--no-cpu-baseline", "--list-sets", str(sets)])
    assert f"{steps} steps of the frame pipeline per graph)" in d["launch"] and f"{sets} list sets" in d["launch"] and d["steps"] == steps
    assert abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    assert d["step_ms"]["p10"] <= d["step_ms"]["median"] <= d["step_ms"]["p90"]


def test_full_line_with_more_steps_than_the_context_has_timing_slots():
    """--full with a K whose per-kernel readings would need more dispatch-packet event pairs than a context holds (4096: 4 x 1100 for the cull
    chain): every reading is bounded (bench.MAX_READING_LAUNCHES), whatever K is, and the line still carries the per-kernel figures."""
    import bench
    d = _run([sys.executable, "bench.py", "--full", "--config", "tiny", "--steps", "1100", "--warmup", "2", "--spinup-ms", "50", "--no-cpu-baseline"])
    assert d["steps"] == 1100 and abs(d["value"] - 128 * 96 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["avg_launch_ms_stats"]["launches"] == bench.MAX_READING_LAUNCHES and r["avg_launch_ms"] > 0
    assert len(r["cull"]["kernels_ms"]) >= 2 and all(v > 0 for v in r["cull"]["kernels_ms"].values())
    assert d["step_ms"]["p10"] <= d["step_ms"]["median"] <= d["step_ms"]["p90"] and d["ms_per_step_dynamic"] > 0


@pytest.mark.parametrize("sets, deferred", [(2, False), (3, False), (3, True), (2, True)])
def test_the_frame_pipeline_graph_leaves_the_frames_results(sets, deferred):
    """The pipeline graph orders two streams by the frames' own dependencies only (shade(k) after cull(k), cull(k + 1) after the shade that last
    read its list set).  Run it with DIFFERENT light sets in the list sets -- a missing dependency would shade a frame from the other frame's lists -- and compare what
    every set holds afterwards with plain stream-ordered launches."""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench
    from sailor_amd import synth
    from sailor_amd.forward_plus import HipContext, ForwardPlus, upload_lights
    dev = torch.device("cuda", 0)
    f = synth.make_frame("C2")
    cam, W, H, N = f.cam, f.cam.width, f.cam.height, len(f.lights)
    side, side2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        ctx, ctx2 = HipContext(dev, stream=side), HipContext(dev, stream=side2)
        d_depth = torch.from_numpy(np.ascontiguousarray(f.depth)).to(dev)
        d_surface = torch.from_numpy(np.ascontiguousarray(f.surface)).to(dev)
        d_l = []
        for p in range(sets):   # the other frames: every light moved
            lights_p = f.lights.copy()
            lights_p["worldPosition"][:, 0] += 3.0 * p
            d_l.append(upload_lights(lights_p, dev))
        fps = [ForwardPlus(ctx, W, H, N) for _ in range(sets)]
        outs = [torch.empty((H, W, 4), dtype=torch.float32, device=dev) for _ in range(sets)]
        ref = []
        for p in range(sets):   # reference: stream order, one frame after the other
            fps[p].cull(cam.frame, d_l[p], N, d_depth)
            fps[p].shade(cam.frame, d_surface, d_l[p], N, None, out=outs[p])
            torch.cuda.synchronize()
            g, idx = fps[p].lists_to_host()
            ref.append((g, idx, outs[p].cpu().numpy().copy()))
            outs[p].zero_()
        assert all(not np.array_equal(ref[0][1], ref[p][1]) for p in range(1, sets))
        torch.cuda.synchronize()
        for p in range(sets):   # (a missing pack, or one that ran before its cull, would leave these)
            fps[p].grid.fill_(-3); fps[p].culled.fill_(-3)
        # deferred: the culls stop after the per-tile lists (which the shades read) and k1_pack follows on the cull's stream, behind the event the
        # shade waits for (the form bench.py launches; a third stream for it crashes hipGraph capture on this stack: scripts/pipeline3_probe.py)
        graph = bench.capture_frame_pipeline(side, side2, 6,
                                             [lambda p=p: fps[p].shade(cam.frame, d_surface, d_l[p], N, None, out=outs[p]) for p in range(sets)],
                                             [lambda p=p: fps[p].cull(cam.frame, d_l[p], N, d_depth, ctx=ctx2, defer_pack=deferred) for p in range(sets)],
                                             None, [lambda p=p: fps[p].pack(ctx2) for p in range(sets)] if deferred else None, side2)
        fps[0].cull(cam.frame, d_l[0], N, d_depth)   # the prologue: frame 0's lists
        torch.cuda.synchronize()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        for p in range(sets):
            g, idx = fps[p].lists_to_host()
            np.testing.assert_array_equal(g, ref[p][0])
            np.testing.assert_array_equal(idx, ref[p][1])
            np.testing.assert_array_equal(outs[p].cpu().numpy(), ref[p][2])
