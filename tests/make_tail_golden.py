"""Writes tests/golden/tiny_tail.npz: the inputs and the Ref32 output of one motion-blur and one LIGHT_TILES case at 32 x 24, as bit patterns.
Run from the repository root: python tests/make_tail_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import tail_cases as tc   # noqa: E402
import tail_ref as ref    # noqa: E402
from sailor_amd import synth   # noqa: E402

W, H = 32, 24
PARAMS = dict(intensity=1.0, samples=5.0, maxSpeed=0.5)

if __name__ == "__main__":
    u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    cam, prev = tc.camera(W, H), tc.camera(W, H, (10.0, 145.0, 0.0), 0.2)
    depth, color = tc.raw_depth(W, H), tc.color_plane(W, H)
    blur = ref.Ref32.motion_blur(cam.frame, prev.frame, depth, color, PARAMS, W, H)
    grid, culled, _ = tc.light_lists(W, H, lengths=[0, 1, 128, 60])
    linear = synth.make_linear_depth(W, H)
    tiles = ref.Ref32.debug_view(cam.frame, ref.LIGHT_TILES, W, H, linear_depth=linear, grid=grid, culled=culled)
    out = ROOT / "tests" / "golden" / "tiny_tail.npz"
    np.savez_compressed(out, frame=np.frombuffer(bytes(cam.frame), np.uint8), previous=np.frombuffer(bytes(prev.frame), np.uint8),
                        params=np.array([PARAMS["intensity"], PARAMS["samples"], PARAMS["maxSpeed"]], np.float32), depth_bits=u32(depth), color_bits=u32(color),
                        blur_bits=u32(blur), grid=grid, culled=culled, linear_bits=u32(linear), tiles_bits=u32(tiles))
    print(out, out.stat().st_size, "bytes")
