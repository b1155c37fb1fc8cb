"""Scenes shared by the tests of the frame's tail (motion blur, Debug view): per case a depth plane, a colour plane, the two frame-data blocks and the
parameters, at 128 x 96 and at the ragged 131 x 77 (H % 16 != 0: the flipped tile rows and the padding term of Debug.shader:124-131 differ from
the aligned case).  Every case carries a note of what it is meant to reach; tests/test_tail_cpu.py checks on the fp32 restatement that it does."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import tail_ref as ref
from hbao_cases import hostile_depth
from sailor_amd import _lib, host, synth

f32 = np.float32
SIZES = ((128, 96), (131, 77))


def camera(width, height, position=(0.0, 150.0, 0.0), yaw=0.0):
    """the synthetic camera (fov 90, zNear 1, zFar 20000) at `position`, turned by `yaw` radians about the up axis"""
    rot = [0.0, float(np.sin(yaw / 2.0)), 0.0, float(np.cos(yaw / 2.0))]
    world = host.transform_matrix(list(position) + [1.0], rot, [1.0, 1.0, 1.0, 1.0])
    cam = synth.Camera(world=world, fov=90.0, z_near=1.0, z_far=20000.0, width=width, height=height)
    cam.frame = host.fill_frame_data(world, cam.fov, cam.z_near, cam.z_far, width, height)
    return cam


def color_plane(width, height, seed=0):
    """an RGBA32F image in [0.25, 4): a smooth ramp plus per-texel noise, so that a tap moved by one texel shows; alpha is not 1 (the pass must write 1)"""
    n = synth.uniforms(synth.STREAM_SURFACE, width * height * 4, 1 << 23, synth.SEED + seed).reshape(height, width, 4)
    x = (np.arange(width, dtype=f32) / f32(width))[None, :, None]
    y = (np.arange(height, dtype=f32) / f32(height))[:, None, None]
    return np.ascontiguousarray((f32(0.25) + f32(1.75) * n + x + y).astype(f32))


def raw_depth(width, height, sky_fraction=0.0):
    return synth.make_raw_depth(synth.make_linear_depth(width, height), 1.0, sky_fraction=sky_fraction)


@dataclass
class BlurCase:
    name: str
    width: int
    height: int
    frame: object
    previous: object
    depth: np.ndarray
    color: np.ndarray
    params: dict = field(default_factory=dict)
    notes: str = ""
    by_class: bool = False   # Ref32 against Ref64 by class (finite, NaN, inf) only


def _blur_case(name, size, notes, position=(0.0, 150.0, 0.0), yaw=0.0, previous="moved", params=None, depth=None, color_size=None, depth_size=None, by_class=False,
               sky_fraction=0.0):
    w, h = size
    cam = camera(w, h)
    if previous == "zero":
        prev = _lib.UboFrameData()
    elif previous == "same":
        prev = cam.frame
    else:
        prev = camera(w, h, position, yaw).frame
    dw, dh = depth_size or size
    cw, ch = color_size or size
    d = raw_depth(dw, dh, sky_fraction) if depth is None else depth
    return BlurCase(name, w, h, cam.frame, prev, d, color_plane(cw, ch), dict(params or {}), notes, by_class)


@lru_cache(maxsize=None)
def blur_cases():
    cases = []
    for size in SIZES:
        tag = "%dx%d" % size
        cases += [
            _blur_case("static_" + tag, size, "static camera: every pixel takes the early-out", previous="same"),
            _blur_case("yaw_" + tag, size, "a small yaw: the ndc shift is theta (1 + x^2), under the early-out bound in the middle of a row and over it at its ends",
                       yaw=0.007),
            _blur_case("dolly_" + tag, size, "a fast dolly sideways and a little upwards, maxSpeed 0.25: min(1, v) binds on x alone where the depth lies between "
                       "Dy / 0.5 and Dx / 0.5, on both axes nearer than that, on none further away", position=(40.0, 160.0, 0.0), params=dict(maxSpeed=0.25, samples=6.0)),
            _blur_case("negative_" + tag, size, "the dolly the other way with maxSpeed 0.0005: a large negative velocity on both axes, unclamped: every tap piles "
                       "up on the 0 edge", position=(-40.0, 110.0, 0.0), params=dict(maxSpeed=0.0005)),
            _blur_case("both_edges_" + tag, size, "x velocity at the cap (u + 1 clamps to 1), y velocity far below 0: taps reach the 1 clamp and the 0 clamp",
                       position=(40.0, 110.0, 0.0), params=dict(maxSpeed=0.0005)),
            _blur_case("first_frame_" + tag, size, "the first frame: previous frame data all zeros, velocity (intensity, intensity) through min(1, NaN)",
                       previous="zero", params=dict(intensity=0.01), by_class=True),
            _blur_case("sky_" + tag, size, "sky blocks: depth 0", yaw=0.02, sky_fraction=0.2),
            _blur_case("hostile_" + tag, size, "hostile depth: 0, 1, denormal, +inf, NaN", yaw=0.02, depth=hostile_depth(*size)[1], by_class=True),
        ]
    w, h = SIZES[0]
    for s in (1.0, 2.0, 10.0, 64.0, 10.7):
        cases.append(_blur_case("samples_%g" % s, SIZES[1], "samples = %g: int(samples) - 1 taps, divided by samples itself" % s, yaw=0.03, params=dict(samples=s)))
    cases.append(_blur_case("extents_differ", (w, h), "colour extent != target extent != depth extent", yaw=0.03, color_size=(97, 61), depth_size=(64, 48)))
    cases.append(_blur_case("shipped_4taps", SIZES[1], "the shipped parameters over a turn that blurs every pixel", yaw=0.05))
    return {c.name: c for c in cases}


# ---- the Debug view --------------------------------------------------------------------------------------------------------------------------
@dataclass
class DebugCase:
    name: str
    width: int
    height: int
    frame: object
    scene: np.ndarray
    linear_depth: np.ndarray
    grid: np.ndarray
    culled: np.ndarray
    ao: np.ndarray
    notes: str = ""


def tiles_of(width, height):
    return (width + ref.TILE - 1) // ref.TILE, (height + ref.TILE - 1) // ref.TILE


def light_lists(width, height, lengths=None):
    """(lightsGrid (tiles, 2) uint32, culledLights uint32[tiles * 128 + 1], the number of lights the view counts per tile): lists of length 0, 1 and 128,
    one cut short by a sentinel in its middle, the others of random length; culledLights[0] is the cull's counter, the lists follow one another"""
    tx, ty = tiles_of(width, height)
    tiles = tx * ty
    rng = np.random.default_rng(width * 1000 + height)
    if lengths is None:
        lengths = rng.integers(0, 40, tiles)
        lengths[:4] = (0, 1, ref.LIGHTS_PER_TILE, 60)
        rng.shuffle(lengths)
    grid = np.zeros((tiles, 2), np.uint32)
    culled = np.full(tiles * ref.LIGHTS_PER_TILE + 1, ref.SENTINEL, np.uint32)
    listed = np.zeros(tiles, np.int64)
    at, cut_done = 1, False
    for t, n in enumerate(lengths):
        n = int(n)
        grid[t] = (at, n)
        culled[at:at + n] = rng.integers(0, 1000, n)
        listed[t] = n
        if n == 60 and not cut_done:      # the sentinel in the middle: the view counts 25 of the 60
            culled[at + 25] = ref.SENTINEL
            listed[t], cut_done = 25, True
        at += n
    culled[0] = at - 1
    return grid, culled, listed


def cascade_depth(width, height, z_far=20000.0):
    """a linear-depth plane that spans every cascade, with texels exactly on each zFar * level[i] bound and one ulp either side of it (rows 2 .. 5)"""
    ld = synth.make_linear_depth(width, height, d_min=10.0, d_max=19000.0).copy()
    for k, level in enumerate(ref.CASCADE_LEVELS):
        bound = f32(z_far) * f32(level)
        ld[2 + k, 8:11] = (np.nextafter(bound, f32(0.0)), bound, np.nextafter(bound, f32(np.inf)))
    ld[8:12, 0:30] = f32(15000.0)   # beyond the last level: NUM_CSM_CASCADES
    return np.ascontiguousarray(ld, f32)


@lru_cache(maxsize=None)
def debug_cases():
    cases = {}
    for w, h in SIZES:
        cam = camera(w, h)
        grid, culled, _ = light_lists(w, h)
        ao = synth.uniforms(synth.STREAM_SURFACE, 64 * 48, 1 << 24).reshape(48, 64).astype(f32)   # another extent than the frame
        cases["%dx%d" % (w, h)] = DebugCase("%dx%d" % (w, h), w, h, cam.frame, color_plane(w - 5, h + 3, seed=1), cascade_depth(w, h), grid, culled,
                                            np.ascontiguousarray(ao), "every mode; scene and g_AO of another extent than the target; lists of length 0, 1, 128 "
                                            "and one cut by a sentinel; depth on and around every cascade bound")
    return cases


def debug_args(case, mode):
    """the keyword arguments Ref32.debug_view reads in this mode"""
    if mode == ref.SCENE:
        return dict(scene=case.scene)
    if mode == ref.AO:
        return dict(ao=case.ao)
    if mode == ref.LIGHT_TILES:
        return dict(linear_depth=case.linear_depth, grid=case.grid, culled=case.culled)
    return dict(scene=case.scene, linear_depth=case.linear_depth)
