"""Launch times of the RenderImGui pass at 3840 x 2160 ("RenderImGui"): k_ui_scan, k_ui_setup and k_ui_blend, by their own dispatch-packet timestamps
(sailor_hip_context_time_launches), over three loads:

  editor  an editor-like frame: one full-screen translucent backdrop, 30 panels of ten rects each (body, title bar, borders, buttons) and about 20 000 glyph
          quads laid out in the panels as lines of text, every panel's text under the panel's clip rect: 150 commands over two draw lists
  layers  64 full-screen translucent layers in one command: 128 triangles over every pixel
  empty   draw data without commands: the call returns before it launches anything (its time is the host's, reported as such)

Every repeat blends over a restored target, so each run does the same arithmetic.  Prints one JSON line with median / p10 / p90 in microseconds.
SAILOR_HIP_LIB selects the library: scripts/build_variant.sh nocmd -DSAILOR_UI_COMMAND_REJECT=0 builds the one without the command-level reject,
scripts/build_variant.sh notile -DSAILOR_UI_TILE_REJECT=0 the one without the per-tile reject.

    python scripts/ui_probe.py [repeats]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sailor_amd import _lib, host  # noqa: E402
from sailor_amd.forward_plus import HipContext, UiPass  # noqa: E402

W, H = 3840, 2160
WHITE_UV = (0.5 / 512, 0.5 / 512)


def atlas(rng):
    """512 x 512: a white texel block at the origin, the rest glyph-like coverage in alpha"""
    t = np.full((512, 512, 4), 255, np.uint8)
    t[..., 3] = rng.integers(0, 256, (512, 512), dtype=np.uint8)
    t[:4, :4] = 255
    return t


def quads(n):
    """n quads' worth of empty vertex and index arrays (4 vertices, 6 indices each), indices relative to the quad's own first vertex + 4 k"""
    v = np.zeros((n, 4), _lib.VERTEX_P2UV2C1_DTYPE)
    i = (np.arange(n, dtype=np.uint32)[:, None] * 4 + np.array([0, 1, 2, 0, 2, 3], np.uint32)[None, :])
    return v, i


def fill(v, x0, y0, x1, y1, u0, v0, u1, v1, color):
    v["position"][:, 0], v["position"][:, 1], v["position"][:, 2], v["position"][:, 3] = (np.stack([x0, y0], -1), np.stack([x1, y0], -1), np.stack([x1, y1], -1),
                                                                                            np.stack([x0, y1], -1))
    v["uv"][:, 0], v["uv"][:, 1], v["uv"][:, 2], v["uv"][:, 3] = np.stack([u0, v0], -1), np.stack([u1, v0], -1), np.stack([u1, v1], -1), np.stack([u0, v1], -1)
    v["color"][:] = np.asarray(color, np.uint32).reshape(-1, 1)


def editor(rng):
    """-> draw data: list 0 = the backdrop and 15 panels, list 1 = 15 panels; a panel = a command of ten rects and four commands of glyph quads"""
    lists = []
    panels = [(rng.uniform(0, W - 900), rng.uniform(0, H - 700), rng.uniform(500, 900), rng.uniform(400, 700)) for _ in range(30)]
    for part in range(2):
        vs, is_, cmds = [], [], []
        nv = ni = 0

        def add(v, i, clip):
            nonlocal nv, ni
            # 16-bit indices: every command gets its own VtxOffset, as ImGui does when a list outgrows 65 536 vertices
            cmds.append(dict(clip_rect=clip, elem_count=i.size, idx_offset=ni, vtx_offset=nv, callback=0))
            vs.append(v.reshape(-1)); is_.append(i.reshape(-1))
            nv += v.size; ni += i.size

        if part == 0:
            v, i = quads(1)
            fill(v, np.float32([0]), np.float32([0]), np.float32([W]), np.float32([H]), *[np.float32([WHITE_UV[0]])] * 4, host.ui_color(0.02, 0.02, 0.05, 0.4))
            add(v, i, (0, 0, W, H))
        for px, py, pw, ph in panels[15 * part: 15 * part + 15]:
            v, i = quads(10)
            x0 = px + np.float32([0, 0, 0, 0, pw - 1, 0, 10, 110, 210, 310])
            y0 = py + np.float32([0, 0, 0, ph - 1, 0, 24, 30, 30, 30, 30])
            x1 = px + np.float32([pw, pw, 1, pw, pw, pw, 100, 200, 300, 400])
            y1 = py + np.float32([ph, 24, ph, ph, ph, 25, 52, 52, 52, 52])
            w = np.full(10, WHITE_UV[0], np.float32)
            fill(v, x0, y0, x1, y1, w, w, w, w, [host.ui_color(*rng.uniform(0.1, 0.5, 3), a) for a in (0.92, 1, 1, 1, 1, 1, 0.8, 0.8, 0.8, 0.8)])
            add(v, i, (px, py, px + pw, py + ph))
            cols, rows_ = int((pw - 20) // 9), int((ph - 70) // 18)
            n = min(cols * rows_, 668)   # 30 panels x 668 = 20 040 glyphs
            k = np.arange(n)
            gx, gy = px + 10 + 9.0 * (k % cols), py + 60 + 18.0 * (k // cols)
            cell = rng.integers(0, 30, (n, 2)).astype(np.float32)
            for q in range(4):   # four commands a panel (ImGui splits on clip rect changes: child windows, columns)
                sel = slice(q * n // 4, (q + 1) * n // 4)
                m = len(k[sel])
                if m == 0:
                    continue
                v, i = quads(m)
                u0, v0 = (8 + cell[sel, 0] * 16) / 512, (8 + cell[sel, 1] * 16) / 512
                fill(v, gx[sel].astype(np.float32), gy[sel].astype(np.float32), (gx[sel] + 8).astype(np.float32), (gy[sel] + 15).astype(np.float32), u0, v0, u0 + 8 / 512,
                     v0 + 15 / 512, host.ui_color(0.9, 0.9, 0.9, 1.0))
                add(v, i, (px + 4, py + 56, px + pw - 4, py + ph - 4))
        lists.append(dict(vertices=np.concatenate(vs), indices=np.concatenate(is_), cmds=cmds))
    return host.ui_draw_data(lists, (float(W), float(H)))


def layers(rng, n=64):
    v, i = quads(n)
    z, w, h = np.zeros(n, np.float32), np.full(n, W, np.float32), np.full(n, H, np.float32)
    u = np.full(n, WHITE_UV[0], np.float32)
    fill(v, z, z, w, h, u, u, u, u, [host.ui_color(*rng.uniform(0, 1, 3), rng.uniform(0.05, 0.5)) for _ in range(n)])
    return host.ui_draw_data([dict(vertices=v.reshape(-1), indices=i.reshape(-1), cmds=[dict(clip_rect=(0, 0, W, H), elem_count=i.size, idx_offset=0, vtx_offset=0,
                                                                                            callback=0)])], (float(W), float(H)))


def empty():
    return host.ui_draw_data([], (float(W), float(H)))


def measure(ctx, draw_data, image, repeats):
    dev = ctx.device
    flat = host.ui_flatten(draw_data)
    assert (flat["width"], flat["height"]) == (W, H)
    up = UiPass(ctx, W, H)
    up.set_texture(image)
    seed = torch.rand((H, W, 4), dtype=torch.float32, device=dev)
    target = seed.clone()
    up.draw_flat(target, flat, index_bytes=2)   # uploads, reserves, and loads the code objects
    v, i, dc = up._buffers
    c = np.ascontiguousarray(flat["commands"], _lib.UI_COMMAND_DTYPE)
    ctx.synchronize()
    rows, host_us = [], []
    for _ in range(repeats + 3):
        target.copy_(seed)
        ctx.synchronize()
        before, _ = ctx.launch_log(0)
        ctx.time_launches(0, 3)
        t0 = time.perf_counter()
        up.draw(target, v, i, c, dc, flat["scale"], flat["translate"])
        host_us.append((time.perf_counter() - t0) * 1e6)
        ctx.synchronize()
        after, _ = ctx.launch_log(0)
        rows.append([ctx.timed_launch_ms(k) * 1e3 for k in range(3)] if after - before == 3 else [0.0, 0.0, 0.0])
    rows, host_us = np.array(rows[3:]), np.array(host_us[3:])
    stat = lambda a: {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(np.percentile(a, 10)), 1), "p90_us": round(float(np.percentile(a, 90)), 1)}  # noqa: E731
    changed = int((target != seed).any(dim=2).sum().item())
    return {"commands": len(c), "triangles": int((c["indexCount"] // 3).sum()), "launches": int(after - before), "changed_pixels": changed,
            "k_ui_scan": stat(rows[:, 0]), "k_ui_setup": stat(rows[:, 1]), "k_ui_blend": stat(rows[:, 2]), "pass": stat(rows.sum(axis=1)), "host_call": stat(host_us)}


def main() -> int:
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    if not torch.cuda.is_available():
        raise RuntimeError("the probe needs a HIP device")
    ctx = HipContext("cuda:0")
    rng = np.random.default_rng(5)
    image = atlas(rng)
    res = {"extent": [W, H], "repeats": repeats, "device": torch.cuda.get_device_name(0), "library": os.environ.get("SAILOR_HIP_LIB", "default"),
           "editor": measure(ctx, editor(rng), image, repeats), "layers": measure(ctx, layers(rng), image, repeats), "empty": measure(ctx, empty(), image, repeats)}
    print(json.dumps(res))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
