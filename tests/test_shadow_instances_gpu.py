"""The shadow pass's per-instance SSBO built on the device (sailor_amd/csrc/shadow_instances.hip) against NumPy -- np.unpackbits(bitorder="little"),
np.nonzero and a fancy-index gather -- exact bytes: out[j] = the model matrix of the j-th set bit of [begin, end), in ascending order, and the count word.

Sizes: 1, 63, 64, 65 (the wave), 4 097, 3 073 = three of the kernel's 1 024-bit chunks plus one bit, and 1 024 * 1 024 + 1 025 bits = more chunks than the
scan kernel's 1 024 threads take in one tile (the carry from tile to tile).  The records are random BIT patterns, so the matrices hold NaNs of every payload,
infinities and denormals; -0.0 and two NaN patterns are planted besides.  Everything is compared as uint32."""
import numpy as np
import pytest
import torch

from sailor_amd import _lib
from sailor_amd.forward_plus import shadow_gather_instances, shadow_gather_instances_batched

pytestmark = pytest.mark.gpu

CHUNK = 1024          # SG_CHUNK of shadow_instances.hip
SIZES = [1, 63, 64, 65, 4097, 3 * CHUNK + 1]
CANARY = 0x5A5AC3C3


def records(n: int, seed: int) -> np.ndarray:
    """n 96-byte PerInstanceData records as uint32 [n, 24]"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 2 ** 32, size=(n, 24), dtype=np.uint64).astype(np.uint32)
    r[0::7, 3] = 0x80000000      # -0.0
    r[0::5, 7] = 0x7FC00001      # a quiet NaN with a payload
    r[0::3, 11] = 0xFF800001     # a signalling NaN, sign set
    return r


def mask_words(n: int, kind: str, seed: int = 0) -> np.ndarray:
    """ceil(n / 64) uint64 words; `n` only sizes the array -- bits past n are set wherever the kind sets them"""
    words = (n + 63) // 64
    if kind == "empty":
        return np.zeros(words, np.uint64)
    if kind == "full":
        return np.full(words, 2 ** 64 - 1, np.uint64)
    if kind == "last":
        m = np.zeros(words, np.uint64)
        m[(n - 1) // 64] = np.uint64(1) << np.uint64((n - 1) % 64)
        return m
    if kind == "alternating":
        m = np.zeros(words, np.uint64)
        m[0::2] = 2 ** 64 - 1
        return m
    rng = np.random.default_rng(seed)
    density = {"sparse": 1 / 64, "dense": 63 / 64, "half": 1 / 2}[kind]
    bits = (rng.random(words * 64) < density).astype(np.uint8)
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def reference(rec: np.ndarray, mask: np.ndarray, begin: int, end: int) -> np.ndarray:
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")
    ids = np.nonzero(bits[begin:end])[0] + begin
    return rec[ids, :16]


def dev(ctx, a: np.ndarray) -> torch.Tensor:
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[a.dtype]
    return torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).to(ctx.device)


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def run_one(ctx, rec_d, rec, mask, begin, end):
    out, count = shadow_gather_instances(ctx, rec_d, dev(ctx, mask), begin, end)
    ref = reference(rec, mask, begin, end)
    assert int(bits_of(count)[0]) == len(ref)
    np.testing.assert_array_equal(bits_of(out)[: len(ref)], ref)
    return ref


@pytest.mark.parametrize("n", SIZES)
def test_every_mask_shape_at_every_size(ctx, n):
    rec = records(n, n)
    rec_d = dev(ctx, rec)
    for kind in ("empty", "full", "last", "alternating", "sparse", "dense"):
        ref = run_one(ctx, rec_d, rec, mask_words(n, kind, seed=n), 0, n)
        if kind == "empty":
            assert len(ref) == 0
        if kind in ("full", "dense"):   # the last word's bits past n are set: they are no instances
            assert len(ref) <= n and (kind != "full" or len(ref) == n)
        if kind == "last":
            assert len(ref) == 1 and np.array_equal(ref[0], rec[n - 1, :16])


def test_stray_bits_past_the_end_are_ignored(ctx):
    n = 4097
    rec = records(n, 1)
    rec_d = dev(ctx, rec)
    full = mask_words(n, "full")
    for end in (1, 63, 64, 65, 1000, 1024, 1025, 4096):
        assert len(run_one(ctx, rec_d, rec, full, 0, end)) == end


def test_ranges_that_begin_and_end_inside_a_word(ctx):
    n = 3 * CHUNK + 1
    rec = records(n, 2)
    rec_d = dev(ctx, rec)
    for kind in ("full", "dense", "sparse", "alternating"):
        mask = mask_words(n, kind, seed=9)
        for begin, end in ((5, 6), (37, 59), (37, 64), (37, 101), (70, 70), (33, 2 * CHUNK + 33 + 7), (1023, 1025), (CHUNK + 31, n)):
            run_one(ctx, rec_d, rec, mask, begin, end)


def test_capacity_below_the_count_keeps_the_prefix_and_a_canary(ctx):
    n = 4097
    rec = records(n, 3)
    rec_d = dev(ctx, rec)
    mask = mask_words(n, "dense", seed=4)
    ref = reference(rec, mask, 0, n)
    for capacity in (len(ref) - 1, CHUNK + 3, 1, 0):
        out = torch.full((len(ref) + 8, 16), CANARY, dtype=torch.int32, device=ctx.device).view(torch.float32)
        count = torch.zeros(1, dtype=torch.int32, device=ctx.device)
        shadow_gather_instances_batched(ctx, rec_d, [(dev(ctx, mask), 0, n, out, count, capacity)])
        got = bits_of(out)
        assert int(bits_of(count)[0]) == len(ref)           # still the full count
        np.testing.assert_array_equal(got[:capacity], ref[:capacity])
        assert (got[capacity:] == CANARY).all()             # nothing past `capacity`, the word right behind it first of all


def test_five_jobs_in_one_call_one_of_them_empty(ctx):
    n = 3 * CHUNK + 1
    rec = records(n, 5)
    rec_d = dev(ctx, rec)
    masks = [mask_words(n, kind, seed=6) for kind in ("dense", "sparse", "empty", "alternating", "full")]
    ranges = [(0, n), (17, 2500), (0, n), (CHUNK, CHUNK), (2 * CHUNK - 1, n)]   # (job 2: no bit set; job 3: no bit at all)
    refs = [reference(rec, m, b, e) for m, (b, e) in zip(masks, ranges)]
    outs = [torch.full((len(r) + 1, 16), CANARY, dtype=torch.int32, device=ctx.device).view(torch.float32) for r in refs]
    counts = torch.full((5,), -1, dtype=torch.int32, device=ctx.device)
    jobs = [(dev(ctx, m), b, e, o, counts[k:k + 1], len(r)) for k, (m, (b, e), o, r) in enumerate(zip(masks, ranges, outs, refs))]
    ws = shadow_gather_instances_batched(ctx, rec_d, jobs)
    np.testing.assert_array_equal(bits_of(counts), [len(r) for r in refs])
    assert len(refs[2]) == 0 and len(refs[3]) == 0
    for o, r in zip(outs, refs):
        got = bits_of(o)
        np.testing.assert_array_equal(got[: len(r)], r)
        assert (got[len(r):] == CANARY).all()
    # a second run into fresh buffers, through the same workspace: identical bytes
    outs2 = [torch.zeros_like(o) for o in outs]
    counts2 = torch.zeros_like(counts)
    jobs2 = [(j[0], j[1], j[2], o, counts2[k:k + 1], j[5]) for k, (j, o) in enumerate(zip(jobs, outs2))]
    assert shadow_gather_instances_batched(ctx, rec_d, jobs2, ws) is ws
    assert torch.equal(counts, counts2)
    for o, o2, r in zip(outs, outs2, refs):
        np.testing.assert_array_equal(bits_of(o2)[: len(r)], bits_of(o)[: len(r)])


def test_more_jobs_than_one_launch_carries(ctx):
    """35 jobs: the kernel arguments hold 32, so the call is two launch pairs with separate offsets in the workspace"""
    n = 4 * CHUNK + 77
    rec = records(n, 7)
    rec_d = dev(ctx, rec)
    mask = mask_words(n, "half", seed=8)
    mask_d = dev(ctx, mask)
    ranges = [(k * 61, k * 61 + 40 * (k % 5) + (CHUNK + 9 if k % 11 == 0 else 0)) for k in range(35)]
    refs = [reference(rec, mask, b, e) for b, e in ranges]
    outs = [torch.zeros((max(len(r), 1), 16), dtype=torch.float32, device=ctx.device) for r in refs]
    counts = torch.full((35,), -1, dtype=torch.int32, device=ctx.device)
    shadow_gather_instances_batched(ctx, rec_d, [(mask_d, b, e, o, counts[k:k + 1]) for k, ((b, e), o) in enumerate(zip(ranges, outs))])
    np.testing.assert_array_equal(bits_of(counts), [len(r) for r in refs])
    for o, r in zip(outs, refs):
        np.testing.assert_array_equal(bits_of(o)[: len(r)], r)


def test_more_chunks_than_the_scan_takes_in_one_tile(ctx):
    n = CHUNK * 1024 + CHUNK + 1
    rec = records(n, 11)
    rec_d = dev(ctx, rec)
    mask = mask_words(n, "half", seed=12)
    ref = run_one(ctx, rec_d, rec, mask, 3, n - 2)
    assert len(ref) > CHUNK * 400
    out2, count2 = shadow_gather_instances(ctx, rec_d, dev(ctx, mask), 3, n - 2)   # twice: the same bytes
    assert int(bits_of(count2)[0]) == len(ref)
    np.testing.assert_array_equal(bits_of(out2)[: len(ref)], ref)


def test_refused_arguments_launch_nothing(ctx):
    rec_d = dev(ctx, records(64, 13))
    mask_d = dev(ctx, mask_words(128, "full"))
    out = torch.zeros((64, 16), dtype=torch.float32, device=ctx.device)
    count = torch.zeros(1, dtype=torch.int32, device=ctx.device)
    for begin, end in ((3, 2), (0, 65)):
        with pytest.raises(_lib.SailorHipError):
            shadow_gather_instances_batched(ctx, rec_d, [(mask_d, begin, end, out, count)])
    with pytest.raises(_lib.SailorHipError):   # a workspace too small for the range
        job = _lib.ShadowGatherJob(mask_d.data_ptr(), 0, 64, out.data_ptr(), 64, 0, count.data_ptr())
        _lib.check(ctx._lib.sailor_hip_shadow_gather_instances_batched(ctx.handle, rec_d.data_ptr(), 64, job, 1, rec_d.data_ptr(), 0), "gather", ctx.handle)
    ctx.synchronize()
    assert not out.any() and int(count[0]) == 0
