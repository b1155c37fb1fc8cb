"""Writes tests/golden/tiny_effects.npz: the inputs and the Ref32 outputs of one case of each post effect at 32 x 24, as bit patterns (arrays only).
Run from the repository root: python tests/make_effects_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import effects_cases as ec   # noqa: E402
import effects_ref as ref    # noqa: E402

W, H = 32, 24
SRC = (19, 13)     # the blurs' and the aberration's source: another extent than the target
BLIT = (13, 7)     # the blit's destination
GAUSS = dict(blurRadius=4.0)
RADIAL = dict(blurRadius=20.0, blurSampleCount=10.5, blurCenter=(0.4, 0.6))
OFFSET = (0.0225, -0.0345, 0.0455)


def outputs(color, plane):
    """name -> Ref32 output of the golden's five launches"""
    R = ref.Ref32
    return dict(gauss=R.blur(color, GAUSS, ref.HORIZONTAL, W, H), radial=R.blur(color, RADIAL, ref.RADIAL, W, H), aberration=R.chromatic_aberration(color, OFFSET, W, H),
                blit4=R.blit_linear(color, *BLIT), blit1=R.blit_linear(plane, *BLIT))


if __name__ == "__main__":
    u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    color, plane = ec.plane(SRC, 20), ec.one_channel(SRC, 21)
    out = ROOT / "tests" / "golden" / "tiny_effects.npz"
    arrays = {k + "_bits": u32(v) for k, v in outputs(color, plane).items()}
    np.savez_compressed(out, color_bits=u32(color), plane_bits=u32(plane), gauss_radius=np.array([GAUSS["blurRadius"]], np.float32),
                        radial_params=np.array([RADIAL["blurRadius"], RADIAL["blurSampleCount"], *RADIAL["blurCenter"]], np.float32),
                        offset=np.array(OFFSET, np.float32), target=np.array([W, H], np.int32), blit_target=np.array(BLIT, np.int32), **arrays)
    print(out, out.stat().st_size, "bytes")
