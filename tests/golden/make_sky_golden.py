"""Writes tests/golden/tiny_sky.npz from Ref32 of tests/sky_ref.py alone, as float32 bit patterns: the 32 x 32 sky, the 8 x 8 sun and the 48 x 32
compose of the cases `level_synth` and `tele_sun` (tests/sky_cases.py), and the six 16 x 16 faces of `env_default`.
Run from the repository root: python tests/golden/make_sky_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import sky_cases as sc  # noqa: E402
import sky_ref as ref  # noqa: E402

r = ref.Ref32()
out = {}
for name in ("level_synth", "tele_sun"):
    sky, sun, composed = sc.planes(r, sc.case(name))
    out[f"{name}_sky"], out[f"{name}_sun"], out[f"{name}_compose"] = (np.ascontiguousarray(a, np.float32).view(np.uint32) for a in (sky, sun, composed))
    print(f"{name}: sky max {sky.max():.4f}, sun lit {float((sun[..., 0] > 0).mean()):.3f}, compose max {composed.max():.4f}")
_n, position, light = sc.ENV_CASES[0]
faces = np.stack([r.env_face(sc.face_uniforms(r, f, position, light), sc.FACE) for f in range(6)])
out["env_default_faces"] = np.ascontiguousarray(faces, np.float32).view(np.uint32)
print("env_default: face maxima", [round(float(f.max()), 4) for f in faces])
np.savez_compressed(ROOT / "tests" / "golden" / "tiny_sky.npz", **out)
