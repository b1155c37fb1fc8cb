"""Seeded inputs of the bloom tests: HDR `Main` images, node parameters and a synthetic lens-dirt texture (the shipped
Textures/Bokeh__Lens_Dirt_9.jpg needs the asset pipeline; any linear RGBA texels exercise the same fetch).

The Karis average divides every tap by 1 + luma, so a grey pixel never gets past 1 and, with the shipped threshold of 3, only bright SATURATED colours
bloom: the images are low-frequency patches, a share of them saturated and bright, so that the thresholded level 1 has both zero and non-zero texels."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

SHIPPED = dict(threshold=3.0, knee=0.2, bloom_intensity=1.3, dirt_intensity=5.0)  # DefaultRenderer.renderer:298-302


@dataclass
class BloomCase:
    name: str
    width: int
    height: int
    levels: int
    seed: int
    threshold: float = SHIPPED["threshold"]
    knee: float = SHIPPED["knee"]
    bloom_intensity: float = SHIPPED["bloom_intensity"]
    dirt_intensity: float = SHIPPED["dirt_intensity"]
    hostile: bool = False  # a few inf / NaN / negative / denormal texels

    def params(self):
        return dict(threshold=self.threshold, knee=self.knee, bloom_intensity=self.bloom_intensity, dirt_intensity=self.dirt_intensity)


CASES = {c.name: c for c in [
    # 320 x 200: rows 200 -> 100 and columns 320 -> 160 show both effects of the group-wise fp32 index arithmetic; 25 -> 12 is an odd level
    BloomCase("c320x200", 320, 200, 6, seed=11),
    # 270 x 135: 135 -> 67 -> 33 -> 16, odd extents on both axes
    BloomCase("odd270x135", 270, 135, 5, seed=12),
    # 128 x 96: every tap is 2 p + 1 (neither effect); a wide knee so that the quadratic part of the curve is used
    BloomCase("pow2_128x96", 128, 96, 5, seed=13, threshold=1.6, knee=0.6, bloom_intensity=0.7, dirt_intensity=2.0),
    # down to 1 x 1 and below the 8 x 8 group; hostile texels
    BloomCase("hostile72x40", 72, 40, 8, seed=14, hostile=True),
]}
FINITE_CASES = [n for n, c in CASES.items() if not c.hostile]


def make_main(case: BloomCase) -> np.ndarray:
    """[height, width, 4] float32 HDR image, alpha 1"""
    rng = np.random.default_rng(case.seed)
    cw, ch = (case.width + 7) // 8, (case.height + 7) // 8
    base = np.exp(rng.normal(-0.5, 1.0, (ch, cw, 3)))
    hot = rng.random((ch, cw)) < 0.3
    tint = np.where(rng.random((ch, cw, 1)) < 0.5, np.array([0.03, 0.05, 1.0]), np.array([1.0, 0.04, 0.02]))
    base = np.where(hot[..., None], tint * rng.uniform(40.0, 400.0, (ch, cw, 1)), base)
    img = np.kron(base, np.ones((8, 8, 1)))[:case.height, :case.width]
    img = img * rng.uniform(0.8, 1.2, img.shape)
    out = np.ones((case.height, case.width, 4), np.float32)
    out[..., :3] = img.astype(np.float32)
    if case.hostile:
        pts = rng.integers(0, [case.height, case.width], (8, 2))
        vals = [np.inf, np.nan, -np.inf, -3.0, 1e-41, 0.0, 3e38, -0.0]
        for (y, x), v in zip(pts, vals):
            out[y, x, rng.integers(0, 3)] = v
    return out


def make_dirt(seed: int = 7, width: int = 37, height: int = 23) -> np.ndarray:
    """[height, width, 4] float32 in [0, 1): no power of two, so the Repeat wrap and the weights are not special"""
    return np.random.default_rng(seed).random((height, width, 4)).astype(np.float32)
