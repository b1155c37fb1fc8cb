"""Writes tests/golden/tiny_masked.npz: every input of one small case of tests/masked_cases.py (a checker-alpha quad over an opaque one), which of its draws
carry ALPHA_CUTOUT, and the keys and planes tests/masked_ref.py renders; the tests rebuild the scene from the file alone (masked_golden_scene below).
Run from the repository root: python tests/make_masked_golden.py"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import masked_cases as cases   # noqa: E402
import masked_ref              # noqa: E402
import surface_cases as sc     # noqa: E402

PATH = Path(__file__).resolve().parent / "golden" / "tiny_masked.npz"


def masked_golden_scene(g):
    name = cases.GOLDEN_CASE
    s = sc.scene_from_arrays(g, name)
    s["draws"] = [dict(d, alpha_cutout=bool(c)) for d, c in zip(s["draws"], g[f"{name}.cutout"])]
    return s


if __name__ == "__main__":
    name = cases.GOLDEN_CASE
    s = cases.CASES[name][0]()
    r = masked_ref.render(s)
    out = sc.scene_to_arrays(s, name)
    out[f"{name}.cutout"] = np.array([d.get("alpha_cutout", False) for d in s["draws"]], np.uint8)
    out[f"{name}.keys"], out[f"{name}.planes"] = r["keys"], r["planes"]
    np.savez_compressed(PATH, **out)
    print(PATH, PATH.stat().st_size, "bytes")
