"""Cases shared by the tests of the post effects (Blur.shader without EVSM and under RADIAL, ChromaticAberation.shader, the Linear blit), at the smallest
shapes where the kernels can still go wrong: targets of 128 x 96 (whole waves, exact texcoords) and of 131 x 77 (a 3-lane last wave, a 1-row last block,
and an odd width that puts a column on u = 0.5, where the aberration's d is 0), differing source and target extents, a source narrower than the Gauss
kernel, 1 x 1.  Every case carries a note of what it is meant to reach; tests/test_effects_cpu.py checks on the fp32 restatement that it does."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import effects_ref as ref
from tail_cases import color_plane

f32 = np.float32
A, B = (128, 96), (131, 77)
GAUSS_RADII = (0.0, 0.9, 1.0, 2.0, 4.0, 5.0, 11.99, 12.0, 13.0, 20.0, 1e9)
DEFINE_SETS = {"": 0, "HORIZONTAL": ref.HORIZONTAL, "VERTICAL": ref.VERTICAL, "HORIZONTAL VERTICAL": ref.HORIZONTAL | ref.VERTICAL}
RADIAL_COUNTS = (1.0, 2.0, 10.5, 64.0, 256.0)


@dataclass
class Case:
    name: str
    kind: str          # "gauss" | "radial" | "aberration" | "blit"
    width: int         # the target's extent
    height: int
    src: np.ndarray    # (sh, sw, 4) float32, or (sh, sw) for a one-channel blit
    notes: str
    params: dict = field(default_factory=dict)
    defines: str = ""
    clamps: tuple = ()          # the sides ("low", "high") on which at least 64 texels must have a fetch outside [0, 1]
    by_class: bool = False      # Ref32 against Ref64, and the kernel's NaNs, by class only

    @property
    def flags(self):
        f = 0
        for d in self.defines.split():
            f |= dict(HORIZONTAL=ref.HORIZONTAL, VERTICAL=ref.VERTICAL, RADIAL=ref.RADIAL)[d]
        return f


def plane(size, seed=0):
    """an RGBA32F image whose alpha is neither 0 nor 1 (tail_cases.color_plane): the alpha decisions of the passes show"""
    return color_plane(size[0], size[1], seed)


def one_channel(size, seed=0):
    return np.ascontiguousarray(plane(size, seed)[..., 1])


def run(Ref, c, info=False):
    """the restatement `Ref` of case c"""
    if c.kind in ("gauss", "radial"):
        return Ref.blur(c.src, c.params, c.flags, c.width, c.height, info=info)
    if c.kind == "aberration":
        return Ref.chromatic_aberration(c.src, c.params["offset"], c.width, c.height, info=info)
    return Ref.blit_linear(c.src, c.width, c.height, info=info)


def _tag(size):
    return "%dx%d" % size


@lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, kind, size, src, notes, **kw):
        out.append(Case(name, kind, size[0], size[1], src, notes, **kw))

    # ---- Gauss --------------------------------------------------------------------------------------------------------------------------------
    for r in GAUSS_RADII:
        add("gauss_r%g" % r, "gauss", B, plane(B), "radius %g: min(uint(r), 12) = %d steps, HORIZONTAL, odd equal extents" % (r, ref.blur_radius(r)),
            params=dict(blurRadius=r), defines="HORIZONTAL")
    for defines in DEFINE_SETS:
        for size, r in ((A, 4.0), (B, 5.0)):
            add("gauss_%s_%s" % (defines.replace(" ", "+") or "none", _tag(size)), "gauss", size, plane(size, 1),
                "define set {%s}: %s" % (defines, {"": "the diagonal", "HORIZONTAL": "rows", "VERTICAL": "columns", "HORIZONTAL VERTICAL": "every tap at uv"}[defines]),
                params=dict(blurRadius=r), defines=defines)
    add("gauss_r1_128x96", "gauss", A, plane(A), "radius 1 at exact texcoords", params=dict(blurRadius=1.0), defines="VERTICAL")
    add("gauss_r12_128x96", "gauss", A, plane(A), "the full row of twelve weights, whole waves", params=dict(blurRadius=12.0), defines="VERTICAL")
    add("gauss_up_131x77_from_64x48", "gauss", B, plane((64, 48), 2), "source smaller than the target: texelSize is the source's", params=dict(blurRadius=4.0),
        defines="VERTICAL")
    add("gauss_down_70x50_from_131x77", "gauss", (70, 50), plane(B, 2), "source larger than the target", params=dict(blurRadius=5.0), defines="HORIZONTAL")
    for defines in ("HORIZONTAL", "VERTICAL", ""):
        add("gauss_narrow_%s" % (defines or "none"), "gauss", A, plane((8, 6), 3), "a source of 8 x 6 under radius 12: the taps of one pair leave the image on both "
            "sides", params=dict(blurRadius=12.0), defines=defines, clamps=("low", "high"))
    add("gauss_1x1", "gauss", (1, 1), plane((1, 1), 4), "1 x 1 source and target: every tap is the one texel", params=dict(blurRadius=4.0))

    # ---- radial -------------------------------------------------------------------------------------------------------------------------------
    for size in (A, B):
        add("radial_shipped_" + _tag(size), "radial", size, plane(size, 5), "the shipped 20 / 10 / (0.5, 0.5)", params=dict(ref.RADIAL_SHIPPED), defines="RADIAL")
    for n in RADIAL_COUNTS:
        add("radial_count%g" % n, "radial", B, plane(B, 6), "count %g: ceil(count) taps, divided by the count itself" % n,
            params=dict(ref.RADIAL_SHIPPED, blurSampleCount=n), defines="RADIAL")
    add("radial_centre_outside", "radial", B, plane(B, 7), "a centre outside [0, 1] and radius 200: x runs past 1, y below 0",
        params=dict(blurRadius=200.0, blurSampleCount=10.0, blurCenter=(1.7, -0.6)), defines="RADIAL", clamps=("low", "high"))
    add("radial_r1e30", "radial", A, plane(A, 8), "radius 1e30: the coordinates leave the int range, the saturating taps clamp",
        params=dict(blurRadius=1e30, blurSampleCount=10.0, blurCenter=(0.5, 0.5)), defines="RADIAL", clamps=("low", "high"), by_class=True)
    add("radial_H_128x96", "radial", A, plane(A, 9), "RADIAL with HORIZONTAL: the direction has no y", params=dict(ref.RADIAL_SHIPPED, blurCenter=(0.25, 0.5)),
        defines="RADIAL HORIZONTAL")
    add("radial_V_131x77", "radial", B, plane(B, 9), "RADIAL with VERTICAL: the direction has no x", params=dict(ref.RADIAL_SHIPPED, blurCenter=(0.5, 0.75)),
        defines="RADIAL VERTICAL")
    add("radial_up_131x77_from_64x48", "radial", B, plane((64, 48), 10), "source smaller than the target", params=dict(ref.RADIAL_SHIPPED), defines="RADIAL")
    add("radial_down_70x50_from_131x77", "radial", (70, 50), plane(B, 10), "source larger than the target", params=dict(ref.RADIAL_SHIPPED), defines="RADIAL")
    add("radial_1x1", "radial", (1, 1), plane((1, 1), 4), "1 x 1 source and target", params=dict(ref.RADIAL_SHIPPED), defines="RADIAL")

    # ---- chromatic aberration ---------------------------------------------------------------------------------------------------------------------
    for size in (A, B):
        add("aberration_shipped_" + _tag(size), "aberration", size, plane(size, 11), "the shipped offsets", params=dict(offset=ref.ABERRATION_SHIPPED))
        add("aberration_zero_" + _tag(size), "aberration", size, plane(size, 12), "zero offsets: a copy with alpha 1", params=dict(offset=(0.0, 0.0, 0.0)))
    add("aberration_negative", "aberration", B, plane(B, 13), "negative offsets: the taps move towards and past the 1 edges", params=dict(offset=(-1.5, -0.3, -0.02)),
        clamps=("high",))
    add("aberration_above_one", "aberration", A, plane(A, 13), "offsets > 1: the taps run past the 0 edges", params=dict(offset=(1.5, 3.0, 1.01)), clamps=("low",))
    add("aberration_both_edges", "aberration", B, plane((64, 48), 14), "offsets of both signs over a smaller source: r past 0, g past 1",
        params=dict(offset=(2.0, -2.0, 0.5)), clamps=("low", "high"))
    add("aberration_down_70x50_from_131x77", "aberration", (70, 50), plane(B, 14), "source larger than the target", params=dict(offset=ref.ABERRATION_SHIPPED))
    add("aberration_1x1", "aberration", (1, 1), plane((1, 1), 4), "1 x 1: u = 0.5, d = 0", params=dict(offset=ref.ABERRATION_SHIPPED))

    # ---- the Linear blit ---------------------------------------------------------------------------------------------------------------------------
    for ch, make in ((4, plane), (1, one_channel)):
        add("blit_half_c%d" % ch, "blit", (64, 32), make((128, 64), 15), "2 : 1 of power-of-two extents: the 2 x 2 mean, weights exactly 0.5")
        add("blit_down_c%d" % ch, "blit", (33, 20), make(B, 16), "a ragged downscale 131 x 77 -> 33 x 20")
        add("blit_up_c%d" % ch, "blit", B, make((33, 20), 17), "an upscale 33 x 20 -> 131 x 77: the border texels clamp")
        add("blit_1x1_c%d" % ch, "blit", (1, 1), make((1, 1), 4), "1 x 1 source and target")
    add("blit_up_128x96", "blit", A, plane((64, 48), 18), "1 : 2 into whole waves")
    return {c.name: c for c in out}
