"""Writes tests/golden/tiny_bloom.npz: bloom_chain of tests/bloom_ref.py (float32) over a seeded 40 x 24 HDR image with three levels, the shipped
parameters and a 5 x 3 dirt texture -- the input, the dirt and the three levels afterwards as float32 words.
Run from the repository root: python tests/golden/make_bloom_golden.py"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import bloom_ref as ref  # noqa: E402
from bloom_cases import SHIPPED, BloomCase, make_dirt, make_main  # noqa: E402

case = BloomCase("tiny", 40, 24, 3, seed=5)
main, dirt = make_main(case), make_dirt(seed=6, width=5, height=3)
levels = ref.bloom_chain(main, case.levels, dirt=dirt, **SHIPPED)
np.savez_compressed(ROOT / "tests" / "golden" / "tiny_bloom.npz", main=main, dirt=dirt,
                    **{f"level{l}_bits": np.ascontiguousarray(v).view(np.uint32) for l, v in enumerate(levels)})
print("tiny_bloom:", [(v.shape, float(v.max())) for v in levels])
