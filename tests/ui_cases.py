"""Named scenes for the RenderImGui pass (tests/ui_ref.py's scene dicts), each with what it was built to reach: a predicate over the restatement's result.
Frames are 72 x 70: with the blend's bins of 32 x 32 pixels that is two whole bins and a partial one on each axis.  Draw data is built with sailor_amd.host's
UiDrawList (pure Python) and flattened by ui_ref.flatten, the restatement of the reference's loop; test_ui_cpu.py holds sailor_host_ui_flatten to it.

The atlas is 8 x 8 texels whose top-left 2 x 2 are opaque white; WHITE_UV is the corner between those four, so an untextured shape samples exactly 1 whatever
the rounding of its interpolated uv.  Glyph uvs are chosen so that pixel centres map to the quarter points between texel centres, far from a change of taps --
except the case that sits ON texel centres on purpose, which is small enough to stay inside the 2 % of pixels a float64 comparison may leave out."""
import numpy as np

import ui_ref as ref
from sailor_amd.host import UiDrawList, ui_color, ui_draw_data

f32 = np.float32
W, H = 72, 70
NUM_SOUPS = 20
WHITE_UV = (0.125, 0.125)
GOLDEN_CASES = ("golden_panel", "golden_order")


def atlas():
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(64, 256, (8, 8), dtype=np.uint8)
    t[:2, :2] = 255
    return t


ATLAS = atlas()


def seed_target(w=W, h=H):
    """BackBuffer as the Debug view left it: something every untouched pixel must keep"""
    j, i = np.mgrid[0:h, 0:w]
    return np.stack([i / 64.0, j / 64.0, (i + j) / 128.0, np.full_like(i, 0.75, float)], -1).astype(f32)


def dl():
    return UiDrawList(WHITE_UV)


def scene(lists, texture=ATLAS, target=None, rows=(13, 52), index_bytes=2, display_size=(W, H), display_pos=(0.0, 0.0), framebuffer_scale=(1.0, 1.0), w=W, h=H):
    s = ref.scene_from(ui_draw_data(lists, display_size, display_pos, framebuffer_scale), texture, seed_target(w, h) if target is None else target, index_bytes, w, h)
    s["rows"] = rows   # a band that cuts triangles, for the CPU check of any rows
    return s


HALF_RED, HALF_GREEN, HALF_BLUE = ui_color(1, 0, 0, 0.5), ui_color(0, 1, 0, 0.5), ui_color(0, 0, 1, 0.5)
FULL = (0.0, 0.0, float(W), float(H))


def count_is(r, boxes):
    """the fragment count of every pixel is the number of the given half-open pixel boxes (x0, y0, x1, y1) that hold it (predicates see the whole frame)"""
    want = np.zeros((H, W), np.int64)
    for x0, y0, x1, y1 in boxes:
        want[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] += 1
    return np.array_equal(r["count"], want[r["rows"][0]:r["rows"][1]])


def st(r, k):
    return r["stats"].get(k, 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------
def _shared_diagonal():
    return scene([dl().clip(*FULL).rect(10, 8, 50, 40, HALF_RED)])


def _bin_corner():
    return scene([dl().clip(*FULL).rect(20, 20, 44, 44, HALF_RED)])


def _order(names):
    rects = dict(A=(8, 8, 40, 40, HALF_RED), B=(20, 16, 56, 48, HALF_GREEN), C=(28, 4, 48, 60, HALF_BLUE))
    def build():
        l = dl().clip(*FULL)
        for n in names:
            l.rect(*rects[n])
        return scene([l])
    return build


def _chunk_seam(n):
    """n triangles over one bin, all covering its middle: every neighbouring pair is order-sensitive, the pair across each chunk seam included"""
    def build():
        rng = np.random.default_rng(n)
        l = dl().clip(*FULL)
        for k in range(n):
            c = ui_color(*rng.uniform(0, 1, 3), rng.uniform(0.05, 0.4))
            l.triangle((33 + k % 3, 33), (62, 34 + k % 5), (34, 62 - k % 4), c)
        return scene([l], rows=(32, 64))
    return build


def _scissor_bin_edges():
    l = dl()
    for clip in ((32, 32, 64, 64), (31, 31, 33, 33), (33, 1, 63, 31), (0, 63, 72, 65), (64, 0, 72, 70)):
        l.clip(*clip).rect(-5, -5, 80, 80, HALF_GREEN)
    return scene([l])


def _scissor_truncated_difference():
    return scene([dl().clip(3.7, 2, 9.2, 30).rect(0, 0, 40, 40, HALF_RED)])


def _scissor_zero_extent():
    return scene([dl().clip(3.7, 2, 4.5, 30).rect(0, 0, 40, 40, HALF_RED).clip(2, 3.25, 30, 3.75).rect(0, 0, 40, 40, HALF_RED)])


def _clip_empty_and_beyond():
    return scene([dl().clip(10, 10, 10, 20).rect(0, 0, 40, 40, HALF_RED).clip(20, 30, 15, 40).rect(0, 0, 40, 40, HALF_RED)
                  .clip(-50, -50, 500, 500).rect(60, 60, 90, 90, HALF_BLUE).clip(80, 10, 90, 20).rect(0, 0, 72, 70, HALF_RED)])


def _raw_list(vertices, indices, cmds):
    v = np.zeros(len(vertices), ref.VERTEX)
    for k, (p, uv, c) in enumerate(vertices):
        v["position"][k], v["uv"][k], v["color"][k] = p, uv, c
    return dict(vertices=v, indices=np.asarray(indices, np.uint32), cmds=cmds)


def _quad_vertices(x0, y0, x1, y1, c):
    return [((x0, y0), WHITE_UV, c), ((x1, y0), WHITE_UV, c), ((x1, y1), WHITE_UV, c), ((x0, y1), WHITE_UV, c)]


def _cmd(clip, elem_count, idx_offset=0, vtx_offset=0, callback=ref.CALLBACK_NONE):
    return dict(clip_rect=clip, elem_count=elem_count, idx_offset=idx_offset, vtx_offset=vtx_offset, callback=callback)


def _odd_first_index_and_vtx_offset():
    """a filler index in front (IdxOffset 1), a second command whose indices are relative to VtxOffset 4"""
    v = _quad_vertices(4, 4, 30, 30, HALF_RED) + _quad_vertices(20, 20, 60, 50, HALF_GREEN)
    return scene([_raw_list(v, [3, 0, 1, 2, 0, 2, 3, 0, 1, 2, 0, 2, 3], [_cmd(FULL, 6, 1, 0), _cmd(FULL, 6, 7, 4)])])


def _two_lists():
    a = dl().clip(*FULL).rect(4, 4, 30, 30, HALF_RED)
    b = dl().clip(0, 0, 50, 50).rect(20, 20, 60, 60, HALF_GREEN).clip(*FULL).rect(40, 2, 70, 30, HALF_BLUE)
    return scene([a, b])


def _index_past_the_buffer():
    """the middle triangle names vertex 9 of 8: dropped; a VtxOffset that pushes a whole command past the buffer"""
    v = _quad_vertices(4, 4, 30, 30, HALF_RED) + _quad_vertices(20, 20, 60, 50, HALF_GREEN)
    return scene([_raw_list(v, [0, 1, 2, 0, 2, 9, 4, 5, 6, 4, 6, 7, 0, 1, 2], [_cmd(FULL, 12), _cmd(FULL, 3, 12, 7)])])


def _index_count_not_a_multiple_of_three():
    """8 indices: two triangles and two ignored; 5 indices from IdxOffset 6: one triangle and two ignored"""
    v = _quad_vertices(4, 4, 30, 30, HALF_RED) + _quad_vertices(20, 20, 60, 50, HALF_GREEN)
    return scene([_raw_list(v, [0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7], [_cmd(FULL, 8), _cmd(FULL, 5, 6)])])


def _both_windings_and_zero_area():
    v = _quad_vertices(10, 10, 40, 40, HALF_RED)
    return scene([_raw_list(v, [0, 1, 2, 0, 3, 2, 0, 2, 2, 0, 1, 1], [_cmd(FULL, 12)])])


def _far_and_nan_vertices():
    l = dl().clip(*FULL)
    l.triangle((1.0e7, 5), (10, 5), (10, 30), HALF_RED)            # 256e7 >= 1e9: dropped
    l.triangle((-3.0e6, -2.0e6), (60, 35), (-3.0e6, 2.0e6), HALF_GREEN)   # drawn: millions of pixels long, 7.7e8 in 1/256 pixels
    l.triangle((float("nan"), 5), (40, 5), (40, 30), HALF_BLUE)     # dropped
    l.triangle((5, float("inf")), (40, 5), (40, 30), HALF_BLUE)     # dropped
    l.triangle((50, 40), (70, 40), (60, 60), HALF_BLUE)
    return scene([l])


def _display_pos_and_scale():
    l = dl().clip(100, 50, 136, 85).rect(104, 54, 120, 70, HALF_RED).clip(110.3, 60.2, 130.9, 80.6).rect(100, 50, 136, 85, HALF_GREEN)
    return scene([l], display_size=(36, 35), display_pos=(100.0, 50.0), framebuffer_scale=(2.0, 2.0))


def _glyphs():
    l = dl().clip(*FULL)
    c = ui_color(1, 1, 1, 0.8)
    l.quad(4, 4, 12, 12, (0.25, 0.25), (0.75, 0.75), c)          # inside the atlas: centres at the quarter points between texel centres
    l.quad(40, 8, 44, 12, (0.25, 0.25), (0.75, 0.75), c)          # 4 x 4 pixels over 4 x 4 texels: ON the texel centres
    l.quad(10, 30, 62, 60, (-1.3, -0.6), (2.63, 1.93), ui_color(0.9, 0.8, 1, 0.6))   # outside [0, 1): Repeat
    l.quad(50, 2, 70, 22, (3.0, 3.0), (3.4, 3.4), c)              # a whole number of atlases away
    return scene([l])


def _aa_fringe():
    return scene([dl().clip(*FULL).rect_aa(8.3, 6.7, 60.2, 40.9, ui_color(0.2, 0.7, 1.0, 0.9), 1.0).rect_aa(28, 28, 68, 66, HALF_RED, 1.5)])


def _zero_alpha_over_alpha():
    return scene([dl().clip(*FULL).rect(10, 10, 40, 40, ui_color(1, 1, 1, 0.0))])


def _nan_in_the_target():
    t = seed_target()
    t[20, 20] = np.nan
    t[21, 25, 3] = np.inf
    t[40, 50, 0] = -np.inf
    return scene([dl().clip(*FULL).rect(10, 10, 60, 60, HALF_RED).rect(15, 15, 55, 55, HALF_GREEN)], target=t)


def _callbacks():
    l = dl().clip(*FULL).rect(4, 4, 30, 30, HALF_RED).callback(ref.CALLBACK_RESET).clip(*FULL).rect(20, 20, 60, 50, HALF_GREEN)
    l.callback(ref.CALLBACK_USER).clip(0, 0, 50, 70).rect(40, 2, 70, 30, HALF_BLUE)
    return scene([l])


def _zero_commands():
    return scene([])


def _no_texels():
    return scene([dl().clip(*FULL).rect(10, 10, 40, 40, HALF_RED)], texture=None)


def _band_cut():
    l = dl().clip(*FULL).triangle((5, 2), (70, 30), (20, 68), [HALF_RED, HALF_GREEN, HALF_BLUE]).triangle((60, 1), (66, 69), (40, 40), HALF_GREEN)
    return scene([l], rows=(17, 47))


def _golden(names):
    """33 x 20, over a zero target: small enough for the golden file"""
    def build():
        l = dl().clip(0, 0, 33, 20).rect(0, 0, 33, 20, ui_color(0.1, 0.2, 0.3, 1.0))
        if "panel" in names:
            l.clip(2.5, 1.5, 30.2, 18.9).rect_aa(4, 3, 28, 17, ui_color(0.9, 0.5, 0.2, 0.7)).quad(6, 5, 14, 13, (0.25, 0.25), (0.75, 0.75), ui_color(1, 1, 1, 0.8))
            l.quad(16, 5, 26, 15, (-0.4, 0.3), (1.7, 1.2), ui_color(0.5, 1, 0.5, 0.5))
        else:
            l.rect(3, 3, 20, 14, HALF_RED).rect(10, 6, 30, 18, HALF_GREEN).rect(14, 1, 24, 19, HALF_BLUE)
        return scene([l], target=np.zeros((20, 33, 4), f32), rows=(5, 16), display_size=(33, 20), w=33, h=20)
    return build


def _inside(r, s, box):
    x0, y0, x1, y1 = box
    return r["count"][y0:y1, x0:x1]


CASES = {
    "shared_diagonal": (_shared_diagonal, lambda r, s: count_is(r, [(10, 8, 50, 40)])),
    "bin_corner": (_bin_corner, lambda r, s: count_is(r, [(20, 20, 44, 44)])),
    "order_abc": (_order("ABC"), lambda r, s: r["count"].max() == 3 and count_is(r, [(8, 8, 40, 40), (20, 16, 56, 48), (28, 4, 48, 60)])),
    "order_cba": (_order("CBA"), lambda r, s: r["count"].max() == 3 and count_is(r, [(8, 8, 40, 40), (20, 16, 56, 48), (28, 4, 48, 60)])),
    "chunk_seam_257": (_chunk_seam(ref.CHUNK + 1), lambda r, s: r["count"].max() == ref.CHUNK + 1 and r["count"][:32, :32].sum() == 0),
    "chunk_seam_513": (_chunk_seam(2 * ref.CHUNK + 1), lambda r, s: r["count"].max() == 2 * ref.CHUNK + 1),
    "scissor_bin_edges": (_scissor_bin_edges, lambda r, s: count_is(r, [(32, 32, 64, 64), (31, 31, 33, 33), (33, 1, 63, 31), (0, 63, 72, 65), (64, 0, 72, 70)])),
    "scissor_truncated_difference": (_scissor_truncated_difference, lambda r, s: list(s["commands"]["scissor"][0]) == [3, 2, 5, 28] and count_is(r, [(3, 2, 8, 30)])),
    "scissor_zero_extent": (_scissor_zero_extent, lambda r, s: len(s["commands"]) == 2 and s["commands"]["scissor"][0][2] == 0 and s["commands"]["scissor"][1][3] == 0
                            and r["count"].sum() == 0),
    "clip_empty_and_beyond": (_clip_empty_and_beyond, lambda r, s: len(s["commands"]) == 1 and list(s["commands"]["scissor"][0]) == [0, 0, W, H]
                              and count_is(r, [(60, 60, 72, 70)])),
    "odd_first_index_and_vtx_offset": (_odd_first_index_and_vtx_offset, lambda r, s: s["commands"]["firstIndex"][0] == 1 and s["commands"]["vertexOffset"][1] == 4
                                       and count_is(r, [(4, 4, 30, 30), (20, 20, 60, 50)])),
    "two_lists": (_two_lists, lambda r, s: list(s["commands"]["firstIndex"]) == [0, 6, 12] and list(s["commands"]["vertexOffset"]) == [0, 4, 4]
                  and count_is(r, [(4, 4, 30, 30), (20, 20, 50, 50), (40, 2, 70, 30)])),
    "index_past_the_buffer": (_index_past_the_buffer, lambda r, s: st(r, "dropped_or_scissored") == 2 and r["count"].max() == 2 and _inside(r, s, (20, 20, 60, 50)).min() >= 1),
    "index_count_not_a_multiple_of_three": (_index_count_not_a_multiple_of_three, lambda r, s: ref.num_triangles(s) == 3 and st(r, "fragments") > 0
                                            and r["count"].max() == 2),
    "both_windings_and_zero_area": (_both_windings_and_zero_area, lambda r, s: st(r, "swapped") == 1 and st(r, "dropped_or_scissored") == 2 and count_is(r, [(10, 10, 40, 40)])),
    "far_and_nan_vertices": (_far_and_nan_vertices, lambda r, s: st(r, "dropped_or_scissored") == 3 and r["count"][:, :50].max() == 1 and r["count"][:, 0].sum() > 0),
    "display_pos_and_scale": (_display_pos_and_scale, lambda r, s: list(s["commands"]["scissor"][1]) == [20, 20, 41, 40] and count_is(r, [(8, 8, 40, 40), (20, 20, 61, 60)])),
    "glyphs": (_glyphs, lambda r, s: count_is(r, [(4, 4, 12, 12), (40, 8, 44, 12), (10, 30, 62, 60), (50, 2, 70, 22)])),
    "aa_fringe": (_aa_fringe, lambda r, s: st(r, "fragments_with_zero_alpha") == 0 and r["count"].max() >= 2),
    "zero_alpha_over_alpha": (_zero_alpha_over_alpha, lambda r, s: st(r, "fragments_with_zero_alpha") == _inside(r, s, (10, 10, 40, 40)).size
                              and (r["target"][20, 10:40, 3] == f32(-0.75)).all() and (r["target"][20, 10:40, :3] == seed_target()[20, 10:40, :3]).all()),
    "nan_in_the_target": (_nan_in_the_target, lambda r, s: np.isnan(r["target"][20, 20]).all() and np.isnan(r["target"]).sum() < 12),
    "callbacks": (_callbacks, lambda r, s: len(s["commands"]) == 3 and count_is(r, [(4, 4, 30, 30), (20, 20, 60, 50), (40, 2, 50, 30)])),
    "zero_commands": (_zero_commands, lambda r, s: len(s["commands"]) == 0 and r["count"].sum() == 0),
    "no_texels": (_no_texels, lambda r, s: st(r, "fragments_with_zero_alpha") == _inside(r, s, (10, 10, 40, 40)).size),
    "band_cut": (_band_cut, lambda r, s: r["count"].max() == 2 and r["count"][s["rows"][0] - 1].sum() > 0 and r["count"][s["rows"][1]].sum() > 0),
    "golden_panel": (_golden("panel"), lambda r, s: r["count"].max() >= 3),
    "golden_order": (_golden("order"), lambda r, s: r["count"].max() == 4),
}


def random_soup(seed):
    """50 to 400 small and large translucent triangles with random uvs, in a handful of commands with random scissors, over two lists"""
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.integers(50, 401))
    lists, left = [], n
    for part in range(2):
        l = dl()
        m = left if part == 1 else left // 2
        while m > 0:
            k = int(min(m, rng.integers(5, 120)))
            if rng.random() < 0.3:
                l.clip(-4.0, -4.0, W + 9.0, H + 9.0)
            else:
                x0, y0 = rng.uniform(-5, W - 10), rng.uniform(-5, H - 10)
                l.clip(x0, y0, x0 + rng.uniform(0.2, W), y0 + rng.uniform(0.2, H))
            for _ in range(k):
                c = rng.uniform([-8, -8], [W + 8, H + 8])
                size = rng.choice([2.0, 6.0, 25.0, 80.0], p=[0.35, 0.35, 0.2, 0.1])
                p = c + rng.uniform(-size, size, (3, 2))
                if rng.random() < 0.2:
                    p = np.round(p)          # vertices on pixel corners: edges through pixel centres' rows and shared edges' ties
                uv = rng.uniform(-1.5, 2.5, (3, 2)) if rng.random() < 0.7 else [WHITE_UV] * 3
                cols = [ui_color(*rng.uniform(0, 1, 3), rng.choice([0.0, 0.25, 0.6, 1.0, rng.uniform(0, 1)])) for _ in range(3)]
                l.triangle(p[0], p[1], p[2], cols, [tuple(q) for q in uv])
            m -= k
        left -= left // 2 if part == 0 else left
        lists.append(l)
    r0 = 3 + seed % 30
    return scene(lists, rows=(r0, r0 + 9 + seed % 25), index_bytes=2 if seed % 2 == 0 else 4)


def all_scenes():
    s = {name: build() for name, (build, _) in CASES.items()}
    for seed in range(NUM_SOUPS):
        s[f"soup_{seed}"] = random_soup(seed)
    return s
