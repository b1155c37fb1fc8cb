"""Regenerates tests/golden/tiny_tonemap.npz: the tiny frame's stored radiance (tests/golden/tiny.npz, the oracle's shade) and what the fp32
restatement of the EyeAdaptation node (tests/eye_adaptation_ref.py) makes of it -- counts, adapted luminance after one frame of 1 / 60 s from
0.5, and the LDR image for the six operator sets.  Arrays only.  Run from the repo root:
    python tests/golden/make_tonemap_golden.py
"""
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
import eye_adaptation_ref as ref  # noqa: E402

DELTA_TIME, INITIAL = 1.0 / 60.0, 0.5


def main() -> None:
    radiance = np.ascontiguousarray(np.load(OUT / "tiny.npz")["radiance"], np.float32)
    out = {"radiance": radiance, "delta_time": np.float32(DELTA_TIME), "initial_luminance": np.float32(INITIAL),
           "constants": np.array(ref.Ref32.constants(radiance.shape[1], radiance.shape[0], DELTA_TIME), np.float32)}
    for ops in ref.OPERATOR_SETS:
        counts, lum, ldr = ref.step(ref.Ref32, radiance, INITIAL, DELTA_TIME, ops)
        out["counts"], out["luminance"] = counts, np.float32(lum)
        out[f"ldr_{ops}"] = ldr
    np.savez_compressed(OUT / "tiny_tonemap.npz", **out)
    print(f"tiny_tonemap: {radiance.shape[1]}x{radiance.shape[0]}, black {int(out['counts'][0])}, luminance {float(out['luminance']):.6f}, "
          f"NaN pixels under LUMINANCE {int(np.isnan(out['ldr_6'][..., 0]).sum())}")


if __name__ == "__main__":
    main()
