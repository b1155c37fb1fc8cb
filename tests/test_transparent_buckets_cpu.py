"""The bucket route of the Transparent queue (sailor_amd/csrc/surface_buckets.hip) without a GPU: the C-ABI's five symbols, their signatures, the version and
sailor_hip_surface_bucket_bytes; the insertion of surf_fragment_bucket (sailor_amd/csrc/surface_masked_body.h) restated as a step machine and run under random
and adversarial schedules, with and without its two shortcuts under STALE loads, with two mutants that must be caught; and every host-side refusal in the
stand-alone scripts/bucket_host_check.cpp, which a test here builds with the host sanitizers and runs."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from sailor_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("sailor_hip_surface_bucket_bytes", "sailor_hip_surface_bucket_begin", "sailor_hip_surface_bucket_draw", "sailor_hip_surface_bucket_draw_gltf",
           "sailor_hip_surface_bucket_layer")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_signatures_version_and_the_size_of_the_store():
    lib = _lib.load()
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    assert lib.sailor_hip_version() >= 13
    for name in ENTRIES:
        kind = "size_t" if name.endswith("_bytes") else "int"
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"SAILOR_HIP_API {kind} {name}(" in header, name
    # the declared argument lists, counted in the header and held against the argtypes
    for name in ENTRIES:
        declared = re.search(rf"{name}\(([^;]*)\);", header).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [3, 9, 18, 18, 11]
    assert _lib.SIGNATURES[ENTRIES[0]][0] is C.c_size_t and all(_lib.SIGNATURES[n][0] is C.c_int for n in ENTRIES[1:])
    u32, sz, i32, P = C.c_uint32, C.c_size_t, C.c_int32, C.c_void_p
    peel = _lib.SIGNATURES["sailor_hip_surface_peel_draw"][1]
    for name in ENTRIES[2:4]:   # _peel_draw's arguments with (dBuckets, bucketBytes, layers) in place of dLast
        assert _lib.SIGNATURES[name][1] == peel[:-1] + [P, sz, u32], name
    assert _lib.SIGNATURES[ENTRIES[1]][1] == [P, i32, i32, C.POINTER(_lib.Band), P, sz, P, sz, u32]
    assert _lib.SIGNATURES[ENTRIES[4]][1] == [P, i32, i32, C.POINTER(_lib.Band), P, sz, P, sz, u32, u32, P]
    # (layers + 1) x rows x width x 8, over the BAND's rows; 0 on a bad argument
    band = _lib.Band(0, 3, 0, 35)
    for layers in (1, 4, 64):
        assert lib.sailor_hip_surface_bucket_bytes(50, band, layers) == (layers + 1) * 35 * 50 * 8
    assert lib.sailor_hip_surface_bucket_bytes(3840, _lib.Band(0, 135, 0, 2160), 4) == 5 * 3840 * 2160 * 8        # the 330 MB of INTEGRATION.md
    assert lib.sailor_hip_surface_bucket_bytes(3840, _lib.Band(0, 135, 0, 2160), 64) == 65 * 3840 * 2160 * 8 > 2 ** 32
    assert lib.sailor_hip_surface_bucket_bytes(50, _lib.Band(1, 2, 16, 7), 4) == 5 * 7 * 50 * 8
    for width, b, layers in ((50, None, 4), (0, band, 4), (-1, band, 4), (32769, band, 4), (50, band, 0), (50, band, 65), (50, band, 2 ** 32 - 1),
                             (50, _lib.Band(0, 3, 0, 0), 4), (50, _lib.Band(0, 3, 0, -5), 4)):
        assert lib.sailor_hip_surface_bucket_bytes(width, b, layers) == 0, (width, layers)
    # what a NULL context reaches
    assert lib.sailor_hip_surface_bucket_begin(None, 8, 8, band, None, 0, None, 0, 4) == -1
    assert lib.sailor_hip_surface_bucket_draw(None, None, None, None, None, 0, None, 0, 0, 8, 8, band, None, 0, None, None, 0, 4) == -1
    assert lib.sailor_hip_surface_bucket_draw_gltf(None, None, None, None, None, 0, None, 0, 0, 8, 8, band, None, 0, None, None, 0, 4) == -1
    assert lib.sailor_hip_surface_bucket_layer(None, 8, 8, band, None, 0, None, 0, 4, 0, None) == -1


def test_the_peel_draws_keep_their_instantiations_and_the_bucket_draws_are_two_more():
    """read from the sources: the body's mode defaults to the Masked queue's, the peel unit asks for SURF_DRAW_PEEL, the bucket unit for SURF_DRAW_BUCKET"""
    csrc = ROOT / "sailor_amd" / "csrc"
    body = (csrc / "surface_masked_body.h").read_text()
    assert "int MODE = SURF_DRAW_MASKED" in body and "enum { SURF_DRAW_MASKED = 0, SURF_DRAW_PEEL = 1, SURF_DRAW_BUCKET = 2 }" in body
    assert re.findall(r"surf_visibility_masked<(\w+), false, (\w+)>", (csrc / "surface_transparent.hip").read_text()) == [("false", "SURF_DRAW_PEEL"), ("true", "SURF_DRAW_PEEL")]
    assert re.findall(r"surf_visibility_masked<(\w+), false, (\w+)>", (csrc / "surface_buckets.hip").read_text()) == [("false", "SURF_DRAW_BUCKET"), ("true", "SURF_DRAW_BUCKET")]
    assert "surface_buckets.o: FLAGS += -fno-slp-vectorize" in (csrc / "Makefile").read_text()


# ---- the insertion as a step machine ------------------------------------------------------------------------------------------------------------------------
EMPTY = 2 ** 64 - 1


class Machine:
    """surf_fragment_bucket's walk over K + 1 slots of one pixel.  One step of one inserter is ONE atomic or ONE plain load.  A slot keeps every value it has
    held: a plain load returns ANY of them (chosen by the random generator) -- a stale value, as a relaxed load beside other waves' atomics may.
    shortcuts: the plane-K reject and the per-plane skip.  The mutants: carry=min carries the smaller of (old, v) on; trust_load takes a load that shows
    v < slot as proof that the atomic will store v and displace what was LOADED: it issues the atomicMin without reading its result and carries the loaded
    value on (or stops, if the load showed EMPTY)."""

    def __init__(self, keys, K, shortcuts, rng, carry=max, trust_load=False):
        self.K, self.shortcuts, self.rng, self.carry, self.trust_load = K, shortcuts, rng, carry, trust_load
        self.slots = [[EMPTY] for _ in range(K + 1)]
        self.ins = [dict(v=int(v), p=0, phase="reject" if shortcuts else "atomic", seen=None) for v in keys]
        self.steps = self.atomics = 0

    def active(self):
        return [i for i, x in enumerate(self.ins) if x["phase"] != "done"]

    def load(self, p):
        h = self.slots[p]
        return h[int(self.rng.integers(0, len(h)))]

    def _next_plane(self, x):
        x["p"] += 1
        x["phase"] = "done" if x["p"] > self.K else ("load" if self.shortcuts else "atomic")

    def step(self, i):
        x = self.ins[i]
        self.steps += 1
        if x["phase"] == "reject":      # a load of the sentinel plane: a full pixel below this key
            x["phase"] = "done" if x["v"] > self.load(self.K) else "load"
        elif x["phase"] == "load":
            seen = self.load(x["p"])
            if x["v"] > seen:
                self._next_plane(x)
            elif self.trust_load:
                x["phase"], x["seen"] = "blind", seen
            else:
                x["phase"] = "atomic"
        else:
            h = self.slots[x["p"]]
            old = h[-1]
            h.append(min(old, x["v"]))
            self.atomics += 1
            if x["phase"] == "blind":
                old = x["seen"]
            if old == EMPTY:
                x["phase"] = "done"
            else:
                x["v"] = self.carry(old, x["v"])
                self._next_plane(x)

    def planes(self):
        return [h[-1] for h in self.slots]


def scheduled(machine, how, rng):
    """runs the machine to its end under a scheduler -> the final planes"""
    turn = 0
    while True:
        act = machine.active()
        if not act:
            return machine.planes()
        if how == "random":
            i = act[int(rng.integers(0, len(act)))]
        elif how == "plane0_first":      # nobody goes on to plane p + 1 before everybody has been through plane p
            i = min(act, key=lambda a: (machine.ins[a]["p"], a))
        elif how == "in_arrival_order":  # one inserter after the other, each to its end
            i = act[0]
        elif how == "last_first":        # ... and the latest arrival first, which is the reverse nesting
            i = act[-1]
        else:                            # round robin, a step each
            i = act[turn % len(act)]
            turn += 1
        machine.step(i)


def keys_of(n, rng):
    """n distinct keys orderPlus1 << 32 | zbits: orders up to 2^32 - 2, among them neighbours, arbitrary depth bits (depth plays no part in the order)"""
    orders = set(int(o) for o in rng.integers(1, 2 ** 32 - 1, n))
    orders |= {2 ** 32 - 2, 2 ** 31, 2 ** 31 - 1, 1}
    orders = rng.permutation(sorted(orders))[:n]
    return [(int(o) << 32) | int(rng.integers(0, 2 ** 32)) for o in orders]


def arrivals(keys, rng):
    """(label, scheduler, arrival order) for one key set: the seeded random schedules and the adversarial ones"""
    asc, desc = sorted(keys), sorted(keys, reverse=True)
    out = [("random", "random", list(keys)), ("random, ascending arrival", "random", asc), ("random, descending arrival", "random", desc),
           ("all at plane 0 first, descending", "plane0_first", desc), ("all at plane 0 first, ascending", "plane0_first", asc),
           ("all at plane 0 first, shuffled", "plane0_first", list(keys)),
           ("descending arrival, one after the other", "in_arrival_order", desc), ("ascending arrival, one after the other", "in_arrival_order", asc),
           ("descending arrival, nested", "last_first", desc), ("round robin, descending", "round_robin", desc), ("round robin, shuffled", "round_robin", list(keys))]
    return out


def expected(keys, K):
    s = sorted(keys)[:K + 1]
    return s + [EMPTY] * (K + 1 - len(s))


def sweep(**mutant):
    """every (n, K, schedule, shortcuts) -> the list of those whose final planes are NOT the K + 1 smallest in ascending order"""
    wrong, runs = [], 0
    for K in (1, 2, 4, 8):
        for n in range(1, 41):
            rng = np.random.default_rng(1000 * K + n)
            keys = keys_of(n, rng)
            for shortcuts in (False, True):
                if mutant.get("trust_load") and not shortcuts:
                    continue
                for label, how, order in arrivals(keys, rng):
                    m = Machine(order, K, shortcuts, rng, **mutant)
                    got = scheduled(m, how, rng)
                    runs += 1
                    assert m.atomics <= n * (K + 1) and m.steps <= 2 * n * (K + 1) + n, "a walk is at most K + 1 atomics and as many loads, and the reject"
                    if got != expected(keys, K):
                        wrong.append((K, n, shortcuts, label))
    return wrong, runs


def test_every_schedule_leaves_the_k_plus_1_smallest_in_ascending_order():
    wrong, runs = sweep()
    assert runs == 4 * 40 * 2 * 11 and not wrong, wrong[:10]


def test_the_shortcuts_save_atomics_and_change_nothing():
    """the same keys in ascending arrival, one after the other, fresh loads: without the shortcuts a fragment of a full pixel pays K + 1 atomics, with them the
    reject takes it with none -- and a typical later fragment pays one atomic, at the first free plane"""
    rng = np.random.default_rng(5)
    keys = sorted(keys_of(40, rng))
    for K in (1, 4, 8):
        plain, short = Machine(keys, K, False, rng), Machine(keys, K, True, rng)
        for m in (plain, short):
            m.load = lambda p, m=m: m.slots[p][-1]   # fresh
            assert scheduled(m, "in_arrival_order", rng) == expected(keys, K)
        assert plain.atomics == sum(min(i, K) + 1 for i in range(40)) and short.atomics == K + 1, (K, plain.atomics, short.atomics)


@pytest.mark.parametrize("mutant", [dict(carry=min), dict(trust_load=True)], ids=["carry_min", "trust_a_stale_load"])
def test_each_mutant_of_the_insertion_is_caught(mutant):
    wrong, runs = sweep(**mutant)
    print(f"{mutant}: {len(wrong)} of {runs} runs differ")
    assert wrong, "the sweep does not catch the mutant"


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_host_side_refusal_in_the_stand_alone_program(tmp_path):
    """scripts/bucket_host_check.cpp -- every refusal of the four entries and the store's size arithmetic, against a context that never reaches a device --
    built as a program of its own with the host sanitizers and run (a few seconds)"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "sailor_amd" / "csrc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc here")
    exe = tmp_path / "bucket_host_check"
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", f"-I{csrc}", str(ROOT / "scripts" / "bucket_host_check.cpp"), "-o", str(exe), f"-L{csrc}", "-lsailor_hip",
                            f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "bucket_host_check: ok" in run.stdout, run.stdout + run.stderr
