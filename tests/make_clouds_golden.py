"""Writes tests/golden/tiny_clouds.npz: the inputs and the Ref32 clouds plane of one tiny case (tests/clouds_cases.py), as bit patterns.
Run from the repository root: python tests/make_clouds_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import clouds_cases as cc   # noqa: E402
from sailor_amd import host   # noqa: E402

CASE = "under_up"

if __name__ == "__main__":
    c = cc.case(CASE)
    sky, plane, exit_step = cc.reference(CASE)
    weather, low, high, noise = cc.textures()
    u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    sun_color = host.sky_sun_color(host.sky_params(lightDirection=c.light).lightDirection[:3])
    out = ROOT / "tests" / "golden" / "tiny_clouds.npz"
    np.savez_compressed(out, case=CASE, weather=weather, low=low, high=high, noise_bits=u32(noise), sky_bits=u32(sky), clouds_bits=u32(plane),
                        exit_step=exit_step, sun_color_bits=u32(sun_color))
    print(out, out.stat().st_size, "bytes")
