"""Writes tests/golden/tiny_ui.npz from tests/ui_ref.py: the inputs and the expected target of the golden cases of tests/ui_cases.py (33 x 20 frames, well
under 32 KB).  tests/test_ui_cpu.py reads it back through the restatement, tests/test_ui_gpu.py through the kernels.  Run from the tests directory."""
from pathlib import Path

import numpy as np

PATH = Path(__file__).resolve().parent / "golden" / "tiny_ui.npz"


def golden_scene(g, name):
    """the scene dict of ui_ref.render from the file's arrays"""
    import ui_ref as ref
    v = np.zeros(len(g[f"{name}.color"]), ref.VERTEX)
    v["position"], v["uv"], v["color"] = g[f"{name}.position"], g[f"{name}.uv"], g[f"{name}.color"]
    c = np.zeros(len(g[f"{name}.commands"]), ref.COMMAND)
    raw = g[f"{name}.commands"]
    c["firstIndex"], c["indexCount"], c["vertexOffset"], c["scissor"] = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3:7]
    W, H, index_bytes = (int(x) for x in g[f"{name}.frame"])
    return dict(W=W, H=H, vertices=v, indices=g[f"{name}.indices"], index_bytes=index_bytes, commands=c, scale=g[f"{name}.push"][:2], translate=g[f"{name}.push"][2:],
                texture=g[f"{name}.texture"], target=g[f"{name}.seed"])


def main():
    import ui_cases as cases
    import ui_ref as ref
    out = {}
    for name in cases.GOLDEN_CASES:
        s = cases.CASES[name][0]()
        r = ref.render(s)
        c = s["commands"]
        out[f"{name}.frame"] = np.array([s["W"], s["H"], s["index_bytes"]], np.int64)
        out[f"{name}.position"], out[f"{name}.uv"], out[f"{name}.color"] = s["vertices"]["position"], s["vertices"]["uv"], s["vertices"]["color"]
        out[f"{name}.indices"] = s["indices"]
        out[f"{name}.commands"] = np.concatenate([c["firstIndex"][:, None], c["indexCount"][:, None], c["vertexOffset"][:, None], c["scissor"]], axis=1).astype(np.int64)
        out[f"{name}.push"] = np.concatenate([s["scale"], s["translate"]]).astype(np.float32)
        out[f"{name}.texture"] = s["texture"]
        out[f"{name}.seed"] = s["target"]
        out[f"{name}.target"] = r["target"]
    np.savez_compressed(PATH, **out)
    print(PATH, PATH.stat().st_size, "bytes")
    assert PATH.stat().st_size < 32 * 1024


if __name__ == "__main__":
    main()
