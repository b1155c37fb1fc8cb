"""GPU suite of the bloom kernels through the C-ABI (sailor_hip_bloom_downscale, sailor_hip_bloom_upscale, sailor_hip_bloom) against the fp32
restatement of tests/bloom_ref.py: finite words BIT FOR BIT, non-finite words by class (NaN, +inf, -inf)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import bloom_ref as ref
from bloom_cases import CASES, SHIPPED, make_dirt, make_main
from sailor_amd import _lib, host
from sailor_amd.forward_plus import Bloom, HipContext

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
F = np.float32


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(ctx.device)


def same(got, want, what):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    ok, msg = ref.same_bits(g.reshape(want.shape), want)
    assert ok, f"{what}: {msg}"


def make_bloom(ctx, c, dirt=None):
    p = host.bloom_params(threshold=c.threshold, knee=c.knee, bloomIntensity=c.bloom_intensity, dirtIntensity=c.dirt_intensity)
    return Bloom(ctx, c.width, c.height, c.levels, params=p, dirt=None if dirt is None else dev(ctx, dirt))


def chain_with_garbage(ctx, b, main):
    """a chain whose level 0 is `main` and whose lower levels hold a value the downscales must overwrite"""
    chain = torch.full((b.chain_floats(),), 1234.5, dtype=torch.float32, device=ctx.device)
    b.level(chain, 0).copy_(dev(ctx, main))
    return chain


@pytest.mark.parametrize("name", list(CASES))
def test_each_entry_point_on_the_restatements_inputs(ctx, name):
    """every downscale (threshold on for level 0 -> 1, off below) and every upscale (mip level 1 with and without dirt, the other levels) on the inputs
    the restatement's chain has at that point"""
    c = CASES[name]
    main, dirt = make_main(c), make_dirt()
    ext = ref.chain_extents(c.width, c.height, c.levels)
    th = ref.push_constants(c.threshold, c.knee)
    with_dirt, no_dirt = make_bloom(ctx, c, dirt), make_bloom(ctx, c)
    lv = [main]
    for i in range(c.levels - 1):
        want = ref.downscale(lv[i], ext[i + 1][0], ext[i + 1][1], th, i == 0)
        chain = torch.full((with_dirt.chain_floats(),), -7.0, dtype=torch.float32, device=ctx.device)
        with_dirt.level(chain, i).copy_(dev(ctx, lv[i]))
        with_dirt.downscale(chain, i)
        ctx.synchronize()
        same(with_dirt.level(chain, i + 1), want, f"{name}: downscale {i} -> {i + 1}")
        same(with_dirt.level(chain, i), lv[i], f"{name}: downscale {i} -> {i + 1} leaves its source alone")
        lv.append(want)
    if not c.hostile:
        assert (lv[1][..., :3] == 0).all(axis=-1).mean() >= 0.05 and (lv[1][..., :3] != 0).any(axis=-1).mean() >= 0.05
    # the threshold off on level 0 -> 1 as well (the entry point takes the flag, the node sets it)
    off = ref.downscale(main, ext[1][0], ext[1][1], th, False)
    out = torch.zeros((ext[1][1], ext[1][0], 4), dtype=torch.float32, device=ctx.device)
    st = ctx._lib.sailor_hip_bloom_downscale(ctx.handle, dev(ctx, main).data_ptr(), c.width, c.height, out.data_ptr(), ext[1][0], ext[1][1],
                                             th.ctypes.data_as(C.POINTER(C.c_float)), 0)
    assert st == 0
    ctx.synchronize()
    same(out, off, f"{name}: downscale 0 -> 1 without the threshold")
    assert not np.array_equal(off, lv[1])
    for i in range(c.levels - 1, 0, -1):
        for b, d in ((with_dirt, dirt), (no_dirt, None)):
            want = ref.upscale(lv[i], lv[i - 1], i, c.bloom_intensity, c.dirt_intensity, d)
            chain = torch.zeros((b.chain_floats(),), dtype=torch.float32, device=ctx.device)
            b.level(chain, i).copy_(dev(ctx, lv[i]))
            b.level(chain, i - 1).copy_(dev(ctx, lv[i - 1]))
            b.upscale(chain, i)
            ctx.synchronize()
            same(b.level(chain, i - 1), want, f"{name}: upscale {i} -> {i - 1}, dirt {d is not None}")
        if i == 1:
            assert not ref.same_bits(ref.upscale(lv[1], lv[0], 1, c.bloom_intensity, c.dirt_intensity, dirt),
                                     ref.upscale(lv[1], lv[0], 1, c.bloom_intensity, c.dirt_intensity, None))[0]
        lv[i - 1] = ref.upscale(lv[i], lv[i - 1], i, c.bloom_intensity, c.dirt_intensity, dirt)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dirty", [True, False])
def test_whole_chain_equals_the_restatement_and_the_launches_one_by_one(ctx, name, dirty):
    c = CASES[name]
    main, dirt = make_main(c), (make_dirt() if dirty else None)
    want = ref.bloom_chain(main, c.levels, dirt=dirt, **c.params())
    b = make_bloom(ctx, c, dirt)
    whole = b.run(chain_with_garbage(ctx, b, main))
    single = chain_with_garbage(ctx, b, main)
    for i in range(c.levels - 1):
        b.downscale(single, i)
    for i in range(c.levels - 1, 0, -1):
        b.upscale(single, i)
    ctx.synchronize()
    for l, w in enumerate(want):
        same(b.level(whole, l), w, f"{name}: level {l} of sailor_hip_bloom")
    assert torch.equal(whole.view(torch.int32), single.view(torch.int32)), "the chain call and the same launches made one by one"
    assert not np.array_equal(want[0], main)


def test_golden_chain(ctx):
    gold = np.load(ROOT / "tests" / "golden" / "tiny_bloom.npz")
    b = Bloom(ctx, 40, 24, 3, dirt=dev(ctx, gold["dirt"]))
    chain = b.run(chain_with_garbage(ctx, b, gold["main"]))
    ctx.synchronize()
    for l in range(3):
        np.testing.assert_array_equal(b.level(chain, l).cpu().numpy().view(np.uint32), gold[f"level{l}_bits"])


def test_captured_and_replayed_chain_equals_the_eager_one(ctx):
    c = CASES["c320x200"]
    mains = [make_main(type(c)(c.name, c.width, c.height, c.levels, seed=200 + i)) for i in range(3)]
    dirt = make_dirt()
    b = make_bloom(ctx, c, dirt)
    eager = [b.run(chain_with_garbage(ctx, b, m)).clone() for m in mains]
    ctx.synchronize()
    assert len({e.cpu().numpy().tobytes() for e in eager}) == 3
    same(b.level(eager[1], 0), ref.bloom_chain(mains[1], c.levels, dirt=dirt, **c.params())[0], "eager frame 1")

    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        b2 = make_bloom(c2, c, dirt)
        inputs = [chain_with_garbage(ctx, b2, m) for m in mains]
        work = [torch.zeros_like(i) for i in inputs]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for i, w in zip(inputs, work):
                w.copy_(i)       # the node rewrites its target in place: every replay starts from the lit frame
                b2.run(w)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for w, e in zip(work, eager):
                assert torch.equal(w.view(torch.int32), e.view(torch.int32))
    finally:
        c2.close()


def test_invalid_arguments_record_nothing(ctx):
    c = CASES["pow2_128x96"]
    b = make_bloom(ctx, c, make_dirt())
    chain = chain_with_garbage(ctx, b, make_main(c))
    before = chain.clone()
    lib, hnd = ctx._lib, ctx.handle
    count = C.c_uint64()
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    launched = count.value
    l0, l1, l2 = (b.level(chain, l).data_ptr() for l in range(3))
    th = host.bloom_push_constants(3.0, 0.2).ctypes.data_as(C.POINTER(C.c_float))
    dn, up, run = lib.sailor_hip_bloom_downscale, lib.sailor_hip_bloom_upscale, lib.sailor_hip_bloom
    assert dn(hnd, None, 128, 96, l1, 64, 48, th, 1) == -1
    assert dn(hnd, l0, 128, 96, None, 64, 48, th, 1) == -1
    assert dn(hnd, l0, 128, 96, l1, 64, 48, None, 1) == -1
    assert dn(hnd, l0, 128, 96, l0, 64, 48, th, 1) == -1            # src == dst
    assert dn(hnd, l0, 128, 96, l1, 63, 48, th, 1) == -1            # not max(1, dim >> 1)
    assert dn(hnd, l0, 128, 96, l1, 64, 49, th, 1) == -1
    assert dn(hnd, l0, 0, 96, l1, 1, 48, th, 1) == -1
    assert dn(hnd, l0 + 4, 128, 96, l1, 64, 48, th, 1) == -1        # planes are float4-aligned
    d = b.dirt.data_ptr()
    assert up(hnd, l1, 64, 48, l0, 128, 96, 1, 1.3, 5.0, d, 37, 0) == -1
    assert up(hnd, l1, 64, 48, l1, 128, 96, 1, 1.3, 5.0, d, 37, 23) == -1
    assert up(hnd, l1, 64, 49, l0, 128, 96, 1, 1.3, 5.0, d, 37, 23) == -1
    assert up(hnd, l2, 32, 24, l0, 128, 96, 2, 1.3, 5.0, d, 37, 23) == -1   # not neighbouring levels
    assert up(hnd, None, 64, 48, l0, 128, 96, 1, 1.3, 5.0, d, 37, 23) == -1
    P = C.byref(b.params)
    assert run(hnd, chain.data_ptr(), 128, 96, 1, P, d, 37, 23) == -1        # levels < 2
    assert run(hnd, chain.data_ptr(), 128, 96, 0, P, d, 37, 23) == -1
    assert run(hnd, None, 128, 96, 5, P, d, 37, 23) == -1
    assert run(hnd, chain.data_ptr(), 128, 96, 5, None, d, 37, 23) == -1
    assert run(hnd, chain.data_ptr(), 128, -96, 5, P, d, 37, 23) == -1
    assert run(hnd, chain.data_ptr(), 128, 96, 5, P, d, -1, 23) == -1
    assert run(None, chain.data_ptr(), 128, 96, 5, P, d, 37, 23) == -1
    lib.sailor_hip_context_launch_log(hnd, C.byref(count), None, 0)
    ctx.synchronize()
    assert count.value == launched, "a refused call launches nothing"
    assert torch.equal(chain.view(torch.int32), before.view(torch.int32))
    # dirt == NULL is accepted: no dirt term
    assert up(hnd, l1, 64, 48, l0, 128, 96, 1, 1.3, 5.0, None, 0, 0) == 0
    ctx.synchronize()


def test_shipped_parameters_are_the_defaults(ctx):
    b = Bloom(ctx, 320, 200)
    assert b.levels == _lib.BLOOM_SHIPPED_LEVELS == 8 and b.extents[-1] == (2, 1)
    assert (b.params.threshold, F(b.params.knee)) == (SHIPPED["threshold"], F(SHIPPED["knee"]))
