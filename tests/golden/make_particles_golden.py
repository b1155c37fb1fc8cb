"""Writes tests/golden/tiny_particles.npz: U1 of tests/particles_cases.py (5 particles x 3 trace frames, 4 frames) -- the records, the constants and, for
frame 3 and frame 0, what is machine-independent of the update: the two record indices of every instance (32-bit unsigned, wrapping), which of them read
the zero record, and isCulled.  (Matrices and colours go through the host's pow / sin / cos / acos and are not stored.)
Run from the repository root: python tests/golden/make_particles_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import particles_cases as cases  # noqa: E402
import particles_ref as ref  # noqa: E402

out = {}
for frame in (3, 0):
    c = cases.u1(frame)
    o = ref.update(c["records"], c["pc"], c["time"])
    out.update({f"frame{frame}_i_new": o["i_new"].astype(np.uint32), f"frame{frame}_i_old": o["i_old"].astype(np.uint32),
                f"frame{frame}_zero_new": o["zero_new"], f"frame{frame}_zero_old": o["zero_old"], f"frame{frame}_is_culled": o["isCulled"]})
pc = c["pc"]
np.savez_compressed(ROOT / "tests" / "golden" / "tiny_particles.npz", records=c["records"].view(np.uint32).reshape(-1, 20),
                    constants=np.array([pc.numInstances, pc.numFrames, pc.fps, pc.traceFrames], np.uint32), trace_decay=np.float32(pc.traceDecay), **out)
print("tiny_particles:", {k: v.tolist() for k, v in out.items() if "i_" in k})
