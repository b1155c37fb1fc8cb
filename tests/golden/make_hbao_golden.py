"""Writes tests/golden/tiny_hbao.npz: Ref32.chain of tests/hbao_ref.py on the raw depth of the `tiny` frame with the shipped parameters and
extents -- HalfDepth as its float32 words, AO / TemporaryR8 / g_AO as the uint8 codes of the R8_UNORM targets.
Run from the repository root: python tests/golden/make_hbao_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import hbao_ref as ref  # noqa: E402
from hbao_cases import noise_texels, raw_depth  # noqa: E402

cam, raw = raw_depth(128, 96)
half, ao, temp, g_ao = ref.Ref32.chain(cam.frame, raw, noise_texels(), ref.SHIPPED, ref.SHIPPED_BLUR, *ref.shipped_extents(128, 96))
np.savez_compressed(ROOT / "tests" / "golden" / "tiny_hbao.npz", half_depth_bits=half.view(np.uint32), ao=ref.codes(ao), temp=ref.codes(temp),
                    g_ao=ref.codes(g_ao))
print(f"tiny_hbao: AO mean {ao.mean():.4f}, {len(np.unique(ref.codes(ao)))} codes; g_AO mean {g_ao.mean():.4f}")
