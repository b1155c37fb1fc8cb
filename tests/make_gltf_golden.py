"""Writes tests/golden/tiny_gltf.npz: every input of a handful of small cases of tests/gltf_cases.py (both shaders in one pass, the normal-matrix models, the
exact cutoffs), the draws' flags, ao_in, and the keys, planes, emissive and ao_out tests/gltf_ref.py renders; the tests rebuild the scenes from the file
alone (gltf_cases.scene_from_arrays).  Run from the repository root: python tests/make_gltf_golden.py"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import gltf_cases as cases   # noqa: E402
import gltf_ref              # noqa: E402

PATH = Path(__file__).resolve().parent / "golden" / "tiny_gltf.npz"
OUTPUTS = ("keys", "planes", "emissive", "ao_out")

if __name__ == "__main__":
    out = {}
    for name in cases.GOLDEN_CASES:
        s = cases.CASES[name][0]()
        r = gltf_ref.render(s)
        out.update(cases.scene_to_arrays(s, name))
        for k in OUTPUTS:
            out[f"{name}.{k}"] = r[k]
    np.savez_compressed(PATH, **out)
    print(PATH, PATH.stat().st_size, "bytes")
