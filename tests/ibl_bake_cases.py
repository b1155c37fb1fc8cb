"""Named inputs of the IBL bakes (sailor_amd/csrc/ibl_prefilter.hip: equirect -> cube, the 2:1 chain, the irradiance map, the specular pre-filter),
shared by tests/test_ibl_bake_cpu.py (C oracle against oracle_f64, closed forms, mutants of the float64 laws) and tests/test_ibl_bake_gpu.py (the kernels
against both).  Everything is small: a float64 irradiance texel costs 65 536 samples, a pre-filter texel 1 024.  The float64 and C-oracle results are
computed once per process and handed out read-only.

The error of an output x against the float64 reference r is measured per texel and colour channel, RELATIVE TO WHAT WAS SUMMED:
    bakes     e = max(|x - r| - t - Q, 0) / a    a = the same float64 bake of |cube| (= |r| unless the cube has a negative texel, where a sum may cancel),
                                                 t = the share of r that rests on face ties (oracle_f64.cube_seam_spread: the sampler does not filter
                                                     across a seam, and a sample ON a seam picks its face by a float's last bit -- one sample of 1 024
                                                     that changes face between two colours is 2e-3 of the texel, which says nothing about a law),
                                                 Q = SUBNORMAL_SLACK: the absolute part of a float rounding, which only the denormal sky can see
    equirect  e = |x - r| / max|image|       per channel: a tap-weight error times the image's steepest step is absolute, not relative to the texel
A kernel passes when its worst e is at most max(2 * the C oracle's worst e on the same case and level, the floor of its own summation tree)."""
import functools

import numpy as np

from oracle import oracle, oracle_f64 as f64

f32 = np.float32
U = 2.0 ** -24   # one float rounding, relative

# ---- the floors: what the kernels' own fixed summation trees may lose, from sailor_amd/csrc/ibl_prefilter.hip -----------------------------------------------
# k_prefilter_env: a lane adds its 16 terms t * cosLi in order (1 rounding for the product, 15 for the adds: the first lands on 0.0f exactly), wave_sum adds
# six shuffle steps: 22 roundings on the way to each colour sum, 21 to the weight (no product), one for the quotient.  Every term is of one sign when the
# texels are, so each rounding is at most U of the final sum: (22 + 21 + 1) U.
PREFILTER_FLOOR = 44 * U
# k_irradiance_map: a lane adds 256 terms (2 t) * cosTheta in order (2 t is exact; 1 + 255 roundings), six shuffle steps, three adds of the four waves'
# partial sums; the division by 65 536 is exact: 265 U.
IRRADIANCE_FLOOR = 265 * U
# k_equirect_to_cube sums nothing: lerp2 is two nested lerps, each (1 - a) rounded, two products, one add -- 4 roundings a level, 8 U of the largest tap
EQUIRECT_FLOOR = 8 * U
# every float operation also rounds by up to half the subnormal spacing, whatever its size: 2^-150 an operation.  A sample is about ten operations below
# the sum (the sampler's three lerps, the product), and the sum of N samples is divided by N (irradiance) or by the sum of cosLi, about N / 2
# (pre-filter): at most 2 * 10 * 2^-150 on a texel, and one more rounding for the quotient itself.  Only the denormal sky can see this term.
SUBNORMAL_SLACK = 32 * 2.0 ** -149

SIZES = [(1, 1), (2, 2), (3, 2), (5, 3), (8, 4), (16, 3), (16, 5), (4, 5), (32, 6)]   # (16, 3) truncated, (4, 5) longer than the chain
CUBES_FINITE = ["smooth", "constant", "six_colours", "sun_centre", "sun_edge", "sun_corner", "level_tagged", "alpha_noise", "negative", "denormals"]
CUBES_NONFINITE = ["nan_texel", "inf_texel", "huge"]
CONSTANT = f32([0.5, 1.25, 2.0, 1.0])
SIX = f32([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1], [1, 0, 1, 1]]) + f32([0.25, 0.25, 0.25, 0])
SUN = f32([1.0e4, 0.8e4, 0.6e4, 1.0])


def level_sizes(size, levels):
    return [max(size >> l, 1) for l in range(levels)]


def level_slices(size, levels):
    """slices of the flat float chain, one per level"""
    offs, total = oracle.cube_level_offsets(size, levels)
    return [slice(offs[l], offs[l + 1] if l + 1 < levels else total) for l in range(levels)]


def _centre_directions(size):
    """unit directions through the texel CENTRES of a size x size x 6 cube (where a texel's value belongs): [6, size, size, 3]"""
    g = (np.arange(size) + 0.5)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    d = np.stack([f64._sampling_vector(gx, gy, face, size) for face in range(6)])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _smooth_level0(size, alpha=1.0):
    d = _centre_directions(size)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = np.empty((6, size, size, 4), f32)
    out[..., 0] = 0.8 + 0.5 * np.sin(3.0 * x + 0.3) * np.cos(2.0 * y) + 0.2 * z
    out[..., 1] = 0.6 + 0.4 * np.cos(2.5 * z - 0.7) * np.sin(1.5 * x + y)
    out[..., 2] = 1.1 + 0.6 * y * y - 0.3 * x * z
    out[..., 3] = alpha
    return out


@functools.lru_cache(maxsize=None)
def cube(name, size, levels):
    """the flat level-major RGBA32F chain of a named cube, read-only"""
    rng = np.random.default_rng(size * 131 + levels)
    sizes, total = level_sizes(size, levels), oracle.cube_level_offsets(size, levels)[1]
    mips = lambda level0: f64.generate_mipmaps_cube(level0, size, levels)
    if name == "smooth":
        chain = mips(_smooth_level0(size))
    elif name == "constant":
        chain = np.tile(CONSTANT, total // 4)
    elif name == "six_colours":   # built directly: every level of a face holds the face's colour
        chain = np.concatenate([np.broadcast_to(SIX[:, None, None, :], (6, s, s, 4)).reshape(-1) for s in sizes]).astype(f32)
    elif name in ("sun_centre", "sun_edge", "sun_corner"):
        l0 = np.full((6, size, size, 4), 0.1, f32)
        l0[..., 3] = 1.0
        y, x = dict(sun_centre=(size // 2, size // 2), sun_edge=(size // 2, size - 1), sun_corner=(0, 0))[name]   # face +X: its right edge borders -Z
        l0[0, y, x] = SUN
        chain = mips(l0)
    elif name == "level_tagged":   # built directly, NOT a mip chain: level l holds l + 1
        chain = np.concatenate([np.tile(f32([l + 1, l + 1, l + 1, 1.0]), 6 * s * s) for l, s in enumerate(sizes)])
    elif name == "alpha_noise":
        l0 = _smooth_level0(size)
        l0[..., 3] = rng.uniform(-2.0, 3.0, (6, size, size))
        chain = mips(l0)
    elif name == "negative":
        l0 = _smooth_level0(size)
        l0[4, size // 3, size // 2, :3] = -50.0
        chain = mips(l0)
    elif name == "denormals":
        chain = mips(_smooth_level0(size) * f32(1e-39))
    elif name in ("nan_texel", "inf_texel"):   # one hostile texel per level, so that every lod meets it
        chain = mips(_smooth_level0(size)).copy()
        for sl, s in zip(level_slices(size, levels), sizes):
            chain[sl].reshape(6, s, s, 4)[2, s // 2, s // 3, :3] = np.nan if name == "nan_texel" else np.inf
    elif name == "huge":
        chain = np.tile(f32([3e38, 3e38, 3e38, 1.0]), total // 4)
    else:
        raise KeyError(name)
    chain = np.ascontiguousarray(chain, f32)
    assert chain.size == total
    chain.setflags(write=False)
    return chain


def ladder(levels):
    """the roughness of level 1 .. levels-1 as sailor_hip_prefilter_env_map and EnvironmentNode.cpp step it, in float"""
    delta = f32(1.0) / f32(max(levels - 1, 1))
    return {level: float(f32(level) * delta) for level in range(1, levels)}


# ---- which cube meets which entry -------------------------------------------------------------------------------------------------------------------------
# pre-filter: every cube at (8, 4) and at the odd (5, 3); the three that read the laws back at every (size, levels)
PREFILTER_CASES = [(c, 8, 4) for c in CUBES_FINITE] + [(c, 5, 3) for c in CUBES_FINITE] + \
                  [(c, s, l) for c in ("smooth", "level_tagged", "sun_corner") for s, l in SIZES if (s, l) not in ((8, 4), (5, 3)) and l > 1
                   and (s == 32) <= (c == "level_tagged")]
PREFILTER_NONFINITE = [(c, 8, 4) for c in CUBES_NONFINITE] + [(c, 5, 3) for c in CUBES_NONFINITE]
HOSTILE_ROUGHNESS = [0.0, 1e-40, 1.0 / 9.0, 0.5, 1.0, 1.5, -0.5]   # and NaN, which is compared by class
HOSTILE_ROUGHNESS_CASES = [("level_tagged", 8, 4, (1, 2, 3)), ("smooth", 5, 3, (0, 1, 2))]   # (cube, size, levels, the levels baked): level 0 too, the direct call allows it
# irradiance (env cube, env size, env levels, output size): lod 0 only, so the chain's length must not matter
IRRADIANCE_F64 = [(c, 8, 4, 3) for c in ("smooth", "sun_edge", "six_colours")] + \
                 [(c, 8, 4, 2) for c in ("sun_centre", "sun_corner", "negative", "alpha_noise", "level_tagged")] + [(c, 8, 4, 1) for c in ("constant", "denormals")] + \
                 [("smooth", 1, 1, 2), ("smooth", 3, 2, 2), ("sun_corner", 5, 3, 3), ("six_colours", 16, 3, 2), ("smooth", 4, 5, 1)]
IRRADIANCE_C = [("smooth", 8, 4, 5), ("sun_centre", 8, 4, 5), ("six_colours", 5, 3, 5)]   # (no float64 here: no sun ON a seam, whose ties it would take to set aside)
IRRADIANCE_NONFINITE = [(c, 8, 4, 2) for c in CUBES_NONFINITE]


def alpha_is_zero(roughness):
    """roughness^2 underflows to 0 in float: the pdf is 0 / 0 or 0 / tiny, see oracle_f64.prefilter_env_level"""
    return float(f32(roughness) * f32(roughness)) == 0.0


def _readonly(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def prefilter_f64(name, size, levels, level, roughness, force_lod=None, magnitude=False):
    """-> (the float64 level [6, s, s, 4], the share of it that rests on face ties)"""
    chain = np.abs(cube(name, size, levels)) if magnitude else cube(name, size, levels)
    with np.errstate(invalid="ignore"):   # an infinite texel times a weight of 0
        return tuple(map(_readonly, f64.prefilter_env_level(chain, size, levels, level, roughness, law=dict(f64.BAKE_LAW, force_lod=force_lod), want_spread=True)))


def prefilter_scale(name, size, levels, level, roughness, force_lod=None):
    return prefilter_f64(name, size, levels, level, roughness, force_lod, name == "negative")[0] if name == "negative" else \
        np.abs(prefilter_f64(name, size, levels, level, roughness, force_lod)[0])


@functools.lru_cache(maxsize=None)
def prefilter_c(name, size, levels, level, roughness):
    """the C oracle's level alone: [6, s, s, 4] float32"""
    import ctypes as C
    raw = cube(name, size, levels)
    out = np.zeros(raw.size, f32)
    oracle.lib().oracle_prefilter_env_level(oracle._p(raw), C.c_int(size), C.c_int(levels), oracle._p(out), C.c_int(level), C.c_float(roughness))
    s = level_sizes(size, levels)[level]
    return _readonly(out[level_slices(size, levels)[level]].reshape(6, s, s, 4).copy())


@functools.lru_cache(maxsize=None)
def irradiance_f64(name, env_size, env_levels, n, magnitude=False):
    """-> (the float64 map [6, n, n, 4], the share of it that rests on face ties)"""
    chain = np.abs(cube(name, env_size, env_levels)) if magnitude else cube(name, env_size, env_levels)
    return tuple(map(_readonly, f64.compute_irradiance_map(chain, env_size, env_levels, n, want_spread=True)))


def irradiance_scale(name, env_size, env_levels, n):
    return irradiance_f64(name, env_size, env_levels, n, True)[0] if name == "negative" else np.abs(irradiance_f64(name, env_size, env_levels, n)[0])


@functools.lru_cache(maxsize=None)
def irradiance_c(name, env_size, env_levels, n):
    return _readonly(oracle.compute_irradiance_map(cube(name, env_size, env_levels), env_size, env_levels, n))


def bake_error(x, ref, scale, spread):
    """worst e over the colour channels (see the module text); x, ref, scale, spread: [..., 4]"""
    err = np.maximum(np.abs(np.asarray(x, np.float64)[..., :3] - ref[..., :3]) - spread[..., :3] - SUBNORMAL_SLACK, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(err == 0.0, 0.0, err / scale[..., :3])
    return float(np.max(e))


def within_c_bound(x, ref, scale, spread, sum_bound, size, chain):
    """what a float evaluation in the shader's order may lose against float64, per texel: `sum_bound` of what was summed (a sequential sum of N terms
    rounds N times), plus its conditioning -- a sample direction carries about 16 roundings, which move a tap weight by 16 U x size and the sample by
    that times the largest step between two texels of the cube, however dark the texel itself is (next to a sun: a lot)"""
    step = np.abs(chain.reshape(-1, 4)[:, :3]).max()
    err = np.abs(np.asarray(x, np.float64)[..., :3] - ref[..., :3]) - spread[..., :3] - SUBNORMAL_SLACK
    return bool((err <= sum_bound * scale[..., :3] + 16 * U * size * step).all())


def roughness_zero_error(x, name, size, levels, level):
    """roughness^2 = 0: a texel reads lod 0 or the last level, by the last bit of dot(N, N) (oracle_f64.prefilter_env_level); the smaller error of the two,
    per texel, and how many texels took each"""
    errs = []
    for lod in (0.0, np.inf):
        ref, spread = prefilter_f64(name, size, levels, level, 0.0, lod)
        scale = prefilter_scale(name, size, levels, level, 0.0, lod)
        e = np.maximum(np.abs(np.asarray(x, np.float64) - ref) - spread - SUBNORMAL_SLACK, 0.0)[..., :3] / scale[..., :3]
        errs.append(e.max(axis=-1))
    return float(np.minimum(*errs).max()), int((errs[0] <= errs[1]).sum())


def allowance(c_err, floor):
    return max(2.0 * c_err, floor)


# ---- panoramas -------------------------------------------------------------------------------------------------------------------------------------------
PANO_SIZES = [(1, 1), (2, 1), (7, 3), (100, 37), (256, 128)]   # (w, h)
PANO_KINDS = ["sun", "tagged"]
EQUIRECT_CUBE_SIZES = [1, 2, 5, 8, 33]


@functools.lru_cache(maxsize=None)
def panorama(kind, w, h):
    """float32 [h, w, 4], read-only.  `sun`: the smooth sky with a sun lobe of tests/test_ibl_prefilter_gpu.py; `tagged`: r = column, g = row, b = a
    checker of the two, alpha = a ramp (the equirect pass interpolates alpha like a colour)"""
    uu, vv = np.meshgrid((np.arange(w, dtype=f32) + 0.5) / w, (np.arange(h, dtype=f32) + 0.5) / h)
    img = np.empty((h, w, 4), f32)
    if kind == "sun":
        rng = np.random.default_rng(3)
        for c in range(3):
            a, b, k = rng.uniform(0.2, 1.0), rng.uniform(0.1, 0.5), rng.integers(1, 4)
            img[..., c] = a + b * np.sin(2 * np.pi * k * uu + c) * np.sin(np.pi * vv) + 20.0 * np.exp(-((uu - 0.3) ** 2 + (vv - 0.25) ** 2) * 400.0)
        img[..., 3] = 1.0
    else:
        col, row = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
        img[..., 0], img[..., 1], img[..., 2], img[..., 3] = col, row, (col + row) % 2, 0.25 + uu + 2.0 * vv
    return _readonly(img)


def covers(w, h, size):
    """the written extents the issue names: the whole face, (w/2, h/3), two empty ones, one beyond the face"""
    return [(size, size), (w // 2, h // 3), (0, h), (w, 0), (size + 7, size + 100)]


EQUIRECT_CASES = [(k, w, h, n, rep) for k in PANO_KINDS for w, h in PANO_SIZES for n in EQUIRECT_CUBE_SIZES for rep in (True, False)]
EQUIRECT_COVER_CASES = [("tagged", 7, 3, 8), ("tagged", 100, 37, 33), ("sun", 256, 128, 33), ("tagged", 2, 1, 5)]   # (kind, w, h, cube size)


@functools.lru_cache(maxsize=None)
def equirect_f64(kind, w, h, n, repeat):
    return _readonly(f64.equirect_to_cube(panorama(kind, w, h), n, repeat=repeat))


@functools.lru_cache(maxsize=None)
def equirect_c(kind, w, h, n, repeat):
    return _readonly(oracle.equirect_to_cube(panorama(kind, w, h), n, repeat=repeat))


def equirect_error(x, ref, img):
    scale = np.maximum(np.abs(img).reshape(-1, 4).max(axis=0), 1e-30)
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref) / scale))
