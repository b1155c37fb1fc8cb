"""The five C-ABI entries of sailor_amd/csrc/ibl_prefilter.hip on the GPU, on the named cases of tests/ibl_bake_cases.py:
  * against the float64 restatements of oracle/oracle_f64.py.  No tolerance is fixed in advance: a kernel's worst error (ibl_bake_cases: relative to what was
    summed, face ties set aside) may be at most max(2 x the C oracle's worst error on the same case and level, the floor of the kernel's own summation tree)
    -- both are float evaluations of the same sums, the factor covers device trigonometry and log2f against libm and the tree order.  Each test prints
    kernel error, C-oracle error and kernel against C oracle.  tests/test_ibl_bake_cpu.py shows that every wrong law breaks this allowance twice over.
  * non-finite texels and a NaN roughness by class against the C oracle;
  * exactness: the 2:1 chain bit for bit, level 0 of the pre-filtered map = the raw level 0, alpha exactly 1 (irradiance, pre-filter) or interpolated (equirect);
  * bounds: 64 canary words behind every output, every input compared with its upload, the per-level call writes its own level only, `cover`;
  * the same call twice gives the same bytes; every refusal branch returns -1 and writes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import ibl_bake_cases as bc
from fuzz_cases import nonfinite_mismatch
from oracle import oracle_f64 as f64

pytestmark = pytest.mark.gpu
f32 = np.float32
CANARY = 0x7FC0DE42   # a quiet NaN with a payload no arithmetic produces
GUARD = 64
INVALID = -1


def _id(case):
    return "-".join(str(v) for v in case)


def upload(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a, f32).reshape(-1).copy()).to(ctx.device)


def unchanged(dev, a):
    return np.array_equal(dev.cpu().numpy().view(np.uint32), np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


class Out:
    """`floats` floats of output, canary-filled, with GUARD canary words behind them"""
    def __init__(self, ctx, floats):
        self.floats = floats
        self.words = torch.full((floats + GUARD,), CANARY, dtype=torch.int32, device=ctx.device)

    def ptr(self, byte_offset=0):
        return C.c_void_p(self.words.data_ptr() + byte_offset)

    def refill(self):
        self.words.fill_(CANARY)

    def read(self):
        """-> the output as float32, after checking the guard"""
        w = self.words.cpu().numpy()
        assert (w[self.floats:] == CANARY).all(), "the words behind the output were written"
        return w[:self.floats].view(f32).copy()

    def untouched(self):
        return bool((self.words.cpu().numpy() == CANARY).all())


def p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def is_canary(a):
    return a.view(np.uint32) == np.uint32(CANARY)


def bake_level(ctx, raw, out, size, levels, level, roughness):
    """sailor_hip_prefilter_env_level into a freshly canary-filled chain: the level as [6, s, s, 4]; every other level must keep its canary"""
    out.refill()
    assert ctx._lib.sailor_hip_prefilter_env_level(ctx.handle, p(raw), out.ptr(), size, levels, level, C.c_float(roughness)) == 0
    ctx.synchronize()
    chain = out.read()
    sl, s = bc.level_slices(size, levels)[level], bc.level_sizes(size, levels)[level]
    mask = np.ones(chain.size, bool)
    mask[sl] = False
    assert is_canary(chain[mask]).all(), f"level {level}: the call wrote another level"
    assert not is_canary(chain[sl]).any()
    return chain[sl].reshape(6, s, s, 4)


# ---- the specular pre-filter, one level per call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.PREFILTER_CASES, ids=_id)
def test_prefilter_level_against_float64(ctx, case):
    name, size, levels = case
    chain = bc.cube(name, size, levels)
    raw, out = upload(ctx, chain), Out(ctx, chain.size)
    for level, roughness in bc.ladder(levels).items():
        got = bake_level(ctx, raw, out, size, levels, level, roughness)
        ref, spread = bc.prefilter_f64(name, size, levels, level, roughness)
        scale, c = bc.prefilter_scale(name, size, levels, level, roughness), bc.prefilter_c(name, size, levels, level, roughness)
        k_err, c_err = bc.bake_error(got, ref, scale, spread), bc.bake_error(c, ref, scale, spread)
        print(f"[prefilter f64] {name} {size}/{levels} level {level} roughness {roughness:.4f}: kernel {k_err:.3e}, C oracle {c_err:.3e}, "
              f"kernel against C oracle {bc.bake_error(got, np.float64(c), scale, spread):.3e}")
        assert np.isfinite(got).all() and k_err <= bc.allowance(c_err, bc.PREFILTER_FLOOR), (level, k_err, c_err)
        np.testing.assert_array_equal(got[..., 3], 1.0)   # whatever the input alpha
    assert unchanged(raw, chain)


@pytest.mark.parametrize("case", bc.HOSTILE_ROUGHNESS_CASES, ids=_id)
def test_prefilter_level_at_hostile_roughness(ctx, case):
    """roughness 0 and a denormal one (alpha = 0: the pdf is 0 / 0 or 0 / tiny, fmaxf drops the NaN -- either lod 0 or the last level, per texel), beyond 1,
    negative, and NaN (no sample passes cosLi > 0: 0 / 0 in every texel, as the shader)"""
    name, size, levels, baked = case
    chain = bc.cube(name, size, levels)
    raw, out = upload(ctx, chain), Out(ctx, chain.size)
    for level in baked:
        for roughness in bc.HOSTILE_ROUGHNESS:
            got = bake_level(ctx, raw, out, size, levels, level, roughness)
            c = bc.prefilter_c(name, size, levels, level, roughness)
            if bc.alpha_is_zero(roughness):
                (k_err, at_lod0), (c_err, _) = bc.roughness_zero_error(got, name, size, levels, level), bc.roughness_zero_error(c, name, size, levels, level)
                against_c = float(np.max(np.abs(np.float64(got) - c)[..., :3] / np.abs(c[..., :3])))
                print(f"[prefilter f64] {name} {size}/{levels} level {level} roughness {roughness:g}: kernel {k_err:.3e} ({at_lod0} of {got[..., 0].size} texels at "
                      f"lod 0), C oracle {c_err:.3e}, kernel against C oracle {against_c:.3e}")
                # both read ONE direction 1 024 times: apart by the C oracle's sequential sum and the kernel's tree at the most -- a texel where the two chose
                # different lods would be apart by the difference between two mip levels
                assert against_c <= 2 * 1024 * bc.U + bc.PREFILTER_FLOOR, "the kernel and the C oracle chose different lods: their dot(N, N) must be the same float"
            else:
                ref, spread = bc.prefilter_f64(name, size, levels, level, roughness)
                scale = bc.prefilter_scale(name, size, levels, level, roughness)
                k_err, c_err = bc.bake_error(got, ref, scale, spread), bc.bake_error(c, ref, scale, spread)
                print(f"[prefilter f64] {name} {size}/{levels} level {level} roughness {roughness:g}: kernel {k_err:.3e}, C oracle {c_err:.3e}, "
                      f"kernel against C oracle {bc.bake_error(got, np.float64(c), scale, spread):.3e}")
            assert np.isfinite(got).all() and k_err <= bc.allowance(c_err, bc.PREFILTER_FLOOR), (level, roughness, k_err, c_err)
            np.testing.assert_array_equal(got[..., 3], 1.0)
        got = bake_level(ctx, raw, out, size, levels, level, float("nan"))
        assert nonfinite_mismatch(got, bc.prefilter_c(name, size, levels, level, float("nan"))) is None
        assert np.isnan(got[..., :3]).all() and (got[..., 3] == 1.0).all()
    assert unchanged(raw, chain)


@pytest.mark.parametrize("case", bc.PREFILTER_NONFINITE, ids=_id)
def test_prefilter_nonfinite_by_class(ctx, case):
    name, size, levels = case
    chain = bc.cube(name, size, levels)
    raw, out = upload(ctx, chain), Out(ctx, chain.size)
    for level, roughness in bc.ladder(levels).items():
        got = bake_level(ctx, raw, out, size, levels, level, roughness)
        c = bc.prefilter_c(name, size, levels, level, roughness)
        assert nonfinite_mismatch(got, c) is None, (level, nonfinite_mismatch(got, c))
        assert (~np.isfinite(got)).any()
        np.testing.assert_array_equal(got[..., 3], 1.0)
    assert unchanged(raw, chain)


# ---- the whole map: the copy, the ladder, levels 1 and 2 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,levels", bc.SIZES)
def test_prefilter_env_map_is_the_copy_and_the_ladder(ctx, size, levels):
    """level 0 is the raw level 0 bit for bit (alpha included); level l is the per-level call at roughness l / max(levels - 1, 1) in float, bit for bit --
    with `levels` 1 nothing but the copy happens, with `levels` 2 level 1 runs at roughness 1; twice the same bytes"""
    chain = bc.cube("alpha_noise", size, levels)
    raw, out, one = upload(ctx, chain), Out(ctx, chain.size), Out(ctx, chain.size)
    runs = []
    for _ in range(2):
        out.refill()
        assert ctx._lib.sailor_hip_prefilter_env_map(ctx.handle, p(raw), out.ptr(), size, levels) == 0
        ctx.synchronize()
        runs.append(out.read())
    got = runs[0]
    np.testing.assert_array_equal(got.view(np.uint32), runs[1].view(np.uint32))
    slices = bc.level_slices(size, levels)
    np.testing.assert_array_equal(got[slices[0]].view(np.uint32), chain[slices[0]].view(np.uint32))
    rungs = bc.ladder(levels)
    assert len(rungs) == levels - 1 and (levels != 2 or rungs[1] == 1.0)
    for level, roughness in rungs.items():
        direct = bake_level(ctx, raw, one, size, levels, level, roughness)
        np.testing.assert_array_equal(got[slices[level]].view(np.uint32), direct.reshape(-1).view(np.uint32))
        np.testing.assert_array_equal(direct[..., 3], 1.0)
    assert unchanged(raw, chain)


# ---- the irradiance map -----------------------------------------------------------------------------------------------------------------------------------
def bake_irradiance(ctx, env, out, env_size, env_levels, n):
    out.refill()
    assert ctx._lib.sailor_hip_compute_irradiance_map(ctx.handle, p(env), env_size, env_levels, out.ptr(), n) == 0
    ctx.synchronize()
    return out.read().reshape(6, n, n, 4)


@pytest.mark.parametrize("case", bc.IRRADIANCE_F64, ids=_id)
def test_irradiance_against_float64(ctx, case):
    name, env_size, env_levels, n = case
    chain = bc.cube(name, env_size, env_levels)
    env, out = upload(ctx, chain), Out(ctx, 6 * n * n * 4)
    got = bake_irradiance(ctx, env, out, env_size, env_levels, n)
    ref, spread = bc.irradiance_f64(*case)
    scale, c = bc.irradiance_scale(*case), bc.irradiance_c(*case)
    k_err, c_err = bc.bake_error(got, ref, scale, spread), bc.bake_error(c, ref, scale, spread)
    print(f"[irradiance f64] {_id(case)}: kernel {k_err:.3e}, C oracle {c_err:.3e}, kernel against C oracle {bc.bake_error(got, np.float64(c), scale, spread):.3e}")
    assert np.isfinite(got).all() and k_err <= bc.allowance(c_err, bc.IRRADIANCE_FLOOR), (k_err, c_err)
    np.testing.assert_array_equal(got[..., 3], 1.0)
    again = bake_irradiance(ctx, env, out, env_size, env_levels, n)
    np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))
    assert unchanged(env, chain)


@pytest.mark.parametrize("case", bc.IRRADIANCE_C, ids=_id)
def test_irradiance_at_an_odd_size_against_the_c_oracle(ctx, case):
    """5 x 5 x 6 texels are too many for float64 here.  Two float evaluations of the same sum, one in sample order, one in the kernel's tree: apart by at
    most the sequential bound plus the tree's floor of what was summed, plus the conditioning of ibl_bake_cases.within_c_bound"""
    name, env_size, env_levels, n = case
    chain = bc.cube(name, env_size, env_levels)
    env, out = upload(ctx, chain), Out(ctx, 6 * n * n * 4)
    got = bake_irradiance(ctx, env, out, env_size, env_levels, n)
    c = np.float64(bc.irradiance_c(*case))
    print(f"[irradiance C] {_id(case)}: kernel against C oracle {float(np.max(np.abs(got - c)[..., :3] / np.abs(c[..., :3]))):.3e}")
    assert np.isfinite(got).all()
    assert bc.within_c_bound(got, c, np.abs(c), np.zeros_like(c), 65536 * bc.U + bc.IRRADIANCE_FLOOR, env_size, chain)
    np.testing.assert_array_equal(got[..., 3], 1.0)
    assert unchanged(env, chain)


@pytest.mark.parametrize("case", bc.IRRADIANCE_NONFINITE, ids=_id)
def test_irradiance_nonfinite_by_class(ctx, case):
    name, env_size, env_levels, n = case
    chain = bc.cube(name, env_size, env_levels)
    env, out = upload(ctx, chain), Out(ctx, 6 * n * n * 4)
    got = bake_irradiance(ctx, env, out, env_size, env_levels, n)
    c = bc.irradiance_c(*case)
    assert nonfinite_mismatch(got, c) is None, nonfinite_mismatch(got, c)
    assert (~np.isfinite(got)).any()
    np.testing.assert_array_equal(got[..., 3], 1.0)
    assert unchanged(env, chain)


# ---- equirect -> cube -------------------------------------------------------------------------------------------------------------------------------------
def convert(ctx, eq, w, h, repeat, out, n, cover):
    out.refill()
    assert ctx._lib.sailor_hip_equirect_to_cube(ctx.handle, p(eq), w, h, 1 if repeat else 0, out.ptr(), n, cover[0], cover[1]) == 0
    ctx.synchronize()
    return out.read().reshape(6, n, n, 4)


@pytest.mark.parametrize("kind,w,h", [(k, w, h) for k in bc.PANO_KINDS for w, h in bc.PANO_SIZES], ids=lambda v: str(v))
def test_equirect_against_float64(ctx, kind, w, h):
    """all four channels: the equirect pass interpolates alpha like a colour"""
    img = bc.panorama(kind, w, h)
    eq = upload(ctx, img)
    for n in bc.EQUIRECT_CUBE_SIZES:
        out = Out(ctx, 6 * n * n * 4)
        for repeat in (True, False):
            got = convert(ctx, eq, w, h, repeat, out, n, (n, n))
            ref, c = bc.equirect_f64(kind, w, h, n, repeat), bc.equirect_c(kind, w, h, n, repeat)
            k_err, c_err = bc.equirect_error(got, ref, img), bc.equirect_error(c, ref, img)
            print(f"[equirect f64] {kind} {w}x{h} -> {n} {'repeat' if repeat else 'clamp'}: kernel {k_err:.3e}, C oracle {c_err:.3e}, "
                  f"kernel against C oracle {bc.equirect_error(got, np.float64(c), img):.3e}")
            assert np.isfinite(got).all() and k_err <= bc.allowance(c_err, bc.EQUIRECT_FLOOR), (n, repeat, k_err, c_err)
            again = convert(ctx, eq, w, h, repeat, out, n, (n, n))
            np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))
    assert unchanged(eq, img)


@pytest.mark.parametrize("case", bc.EQUIRECT_COVER_CASES, ids=_id)
def test_equirect_cover(ctx, case):
    """texels outside the cover keep the canary; an empty cover returns OK and writes nothing; a cover beyond the face is the whole face"""
    kind, w, h, n = case
    img = bc.panorama(kind, w, h)
    eq, out = upload(ctx, img), Out(ctx, 6 * n * n * 4)
    whole = convert(ctx, eq, w, h, True, out, n, (n, n))
    assert not is_canary(whole).any()
    for cover in bc.covers(w, h, n):
        got = [convert(ctx, eq, w, h, True, out, n, cover)]
        cw, ch = min(cover[0], n), min(cover[1], n)
        inside = np.zeros((6, n, n), bool)
        inside[:, :ch, :cw] = True
        assert is_canary(got[0][~inside]).all(), cover
        np.testing.assert_array_equal(got[0][inside].view(np.uint32), whole[inside].view(np.uint32))
        if cw == 0 or ch == 0:
            assert out.untouched(), cover
    assert unchanged(eq, img)


# ---- the 2:1 chain ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,levels", bc.SIZES)
def test_mip_chain_bit_for_bit(ctx, size, levels):
    for name in ("alpha_noise", "sun_corner", "huge"):
        level0 = bc.cube(name, size, levels)[:6 * size * size * 4]
        want = f64.generate_mipmaps_cube(level0, size, levels)
        out = Out(ctx, want.size)
        out.words[:level0.size] = upload(ctx, level0).view(torch.int32)
        runs = []
        for _ in range(2):   # in place: the second run reads the same level 0
            assert ctx._lib.sailor_hip_generate_mipmaps_cube(ctx.handle, out.ptr(), size, levels) == 0
            ctx.synchronize()
            runs.append(out.read())
        np.testing.assert_array_equal(runs[0].view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(runs[1].view(np.uint32), want.view(np.uint32))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_return_invalid_and_write_nothing(ctx):
    """every SAILOR_HIP_ERR_INVALID_ARGUMENT branch of the five entries.  Each is decided on the host before a launch: no bad address is ever handed to a
    kernel (the misaligned pointers lie inside live buffers)."""
    lib, hnd = ctx._lib, ctx.handle
    size, levels, n, w, h = 8, 4, 2, 7, 3
    chain, img = bc.cube("smooth", size, levels), bc.panorama("tagged", w, h)
    raw, eq = upload(ctx, chain), upload(ctx, img)
    env, irr, cube = Out(ctx, chain.size), Out(ctx, 6 * n * n * 4), Out(ctx, 6 * size * size * 4)
    mips = upload(ctx, chain)   # in/out of the chain entry: must stay as uploaded
    rough = C.c_float(0.5)
    valid = {
        "equirect": (lib.sailor_hip_equirect_to_cube, [hnd, p(eq), w, h, 1, cube.ptr(), size, size, size]),
        "mips": (lib.sailor_hip_generate_mipmaps_cube, [hnd, p(mips), size, levels]),
        "irradiance": (lib.sailor_hip_compute_irradiance_map, [hnd, p(raw), size, levels, irr.ptr(), n]),
        "level": (lib.sailor_hip_prefilter_env_level, [hnd, p(raw), env.ptr(), size, levels, 1, rough]),
        "map": (lib.sailor_hip_prefilter_env_map, [hnd, p(raw), env.ptr(), size, levels]),
    }
    bad = {   # argument index -> the values that must be refused
        "equirect": {0: [None], 1: [None, p(eq, 4)], 2: [0, -1, 32769], 3: [0, -1, 32769], 5: [None, cube.ptr(4)], 6: [0, -1, 8193], 7: [-1], 8: [-1]},
        "mips": {0: [None], 1: [None, p(mips, 4)], 2: [0, -1, 8193], 3: [0, -1, 17]},
        "irradiance": {0: [None], 1: [None, p(raw, 4)], 2: [0, -1], 3: [0, -1, 17], 4: [None, irr.ptr(4)], 5: [0, -1, 4097]},
        "level": {0: [None], 1: [None, p(raw, 4), env.ptr()], 2: [None, env.ptr(4)], 3: [0, -1, 8193], 4: [0, 17], 5: [-1, levels, levels + 1]},
        "map": {0: [None], 1: [None, p(raw, 4), env.ptr()], 2: [None, env.ptr(4)], 3: [0, -1, 8193], 4: [0, -1, 17]},
    }
    tried = 0
    for entry, (fn, ok) in valid.items():
        for index, values in bad[entry].items():
            for value in values:
                args = list(ok)
                args[index] = value
                assert fn(*args) == INVALID, (entry, index, value)
                tried += 1
    assert lib.sailor_hip_prefilter_env_level(hnd, p(raw), env.ptr(), size, 0, 0, rough) == INVALID   # levels 0 with the only level it could name
    ctx.synchronize()
    assert tried >= 60
    assert env.untouched() and irr.untouched() and cube.untouched(), "a refused call wrote an output"
    assert unchanged(mips, chain) and unchanged(raw, chain) and unchanged(eq, img)
    # ... and the valid calls are valid
    for entry, (fn, ok) in valid.items():
        assert fn(*ok) == 0, entry
    ctx.synchronize()
    env.read(), irr.read(), cube.read()
