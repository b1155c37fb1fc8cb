"""Writes tests/golden/tiny_stars.npz: one Ref32 output of each kernel of sailor_amd/csrc/sky_stars.hip (tests/stars_cases.py) and of the host functions,
as bit patterns.  The inputs are the cases' own (seeded, or the committed BSC5 and stars_color_rows.npy).
Run from the repository root: python tests/make_stars_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import stars_cases as sc   # noqa: E402
import stars_ref as sref   # noqa: E402

SHAFTS, STARS = "in_view_60", "synthetic_96"

if __name__ == "__main__":
    r = sref.Ref32()
    u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    shafts = sc.shaft_reference(SHAFTS)[0]
    stars, S = sc.star_reference(STARS)
    positions, colors, _ = sc.fixture_mesh()
    table = r.color_table(sc.color_rows())
    out = ROOT / "tests" / "golden" / "tiny_stars.npz"
    np.savez_compressed(out, shafts_case=SHAFTS, stars_case=STARS, shafts_bits=u32(shafts), stars_bits=u32(stars), pixels=(S["py"] * 96 + S["px"]).astype(np.int32),
                        drop=S["drop"].astype(np.int32), table_bits=u32(table), first_positions_bits=u32(positions[:64]), first_colors_bits=u32(colors[:64]),
                        model_bits=u32(r.stars_model((10.0, 150.0, -20.0))))
    print(out, out.stat().st_size, "bytes")
