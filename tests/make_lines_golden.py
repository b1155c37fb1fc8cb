"""Writes tests/golden/tiny_lines.npz from tests/lines_ref.py: the inputs and the expected keys, Main and DepthBuffer of a few cases of tests/lines_cases.py (a
few KB).  tests/test_lines_cpu.py reads it back through the restatement, tests/test_lines_gpu.py through the kernels.  Run from the tests directory."""
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "golden" / "tiny_lines.npz"


def golden_scene(g, name):
    """the scene dict of lines_ref.render from the file's arrays"""
    import lines_ref as ref
    v = np.zeros(len(g[f"{name}.vertices"]), ref.VERTEX)
    v["position"], v["color"] = g[f"{name}.vertices"][:, :3], g[f"{name}.vertices"][:, 3:]
    W, H, prim_base = (int(x) for x in g[f"{name}.frame"])
    return dict(W=W, H=H, vp=g[f"{name}.vp"], vertices=v, indices=None, prim_base=prim_base, depth=g[f"{name}.depth"], target=g[f"{name}.seed"])


def main():
    import lines_cases as cases
    import lines_ref as ref
    out = {}
    for name in cases.GOLDEN_CASES:
        s = cases.CASES[name][0]()
        assert s["indices"] is None
        r = ref.render(s)
        out[f"{name}.frame"] = np.array([s["W"], s["H"], s["prim_base"]], np.int64)
        out[f"{name}.vp"] = s["vp"]
        out[f"{name}.vertices"] = np.concatenate([s["vertices"]["position"], s["vertices"]["color"]], axis=1)
        out[f"{name}.depth"] = np.zeros((s["H"], s["W"]), np.float32) if s["depth"] is None else s["depth"]
        out[f"{name}.seed"] = s["target"]
        out[f"{name}.keys"], out[f"{name}.target"], out[f"{name}.depth_out"] = r["keys"], r["target"], r["depth"]
    np.savez_compressed(PATH, **out)
    print(PATH, PATH.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
