"""Writes tests/golden/tiny_surface.npz: every input (frame, matrices, instances, materials, textures, draws), the keys and the planes of three small cases of
tests/surface_cases.py as tests/surface_ref.py renders them; the tests rebuild the scenes from the file alone (surface_cases.scene_from_arrays).
Run from the repository root: python tests/make_surface_golden.py"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import surface_cases as cases  # noqa: E402
import surface_ref as ref      # noqa: E402

out = {}
for name in cases.GOLDEN_CASES:
    s = cases.CASES[name][0]()
    r = ref.render(s)
    out.update(cases.scene_to_arrays(s, name))
    out[f"{name}.keys"], out[f"{name}.planes"] = r["keys"], r["planes"]
path = Path(__file__).resolve().parent / "golden" / "tiny_surface.npz"
np.savez_compressed(path, **out)
print(path, path.stat().st_size, "bytes")
