"""The RenderImGui pass without a GPU: tests/ui_ref.py (the float32 restatement of the rules in include/sailor_hip.h) against the golden file, its float64
twin and its reverse-order mutant; every case of tests/ui_cases.py against the predicate it was built for; a band against the rows of the whole frame;
sailor_host_ui_flatten against the Python restatement of Submodules/ImGuiApi.cpp:118-125 and :197-275; the ABI; the node's registration and its place in the
shipped renderer."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ui_cases as cases
import ui_ref as ref
from make_ui_golden import PATH as GOLDEN, golden_scene

# The worst |float32 - float64| of a colour channel over every case and soup, on the pixels where both pick the same texels in every fetch (measured, and
# recorded in DESIGN.md, "RenderImGui"): soup_0, chains of dozens of blends over colours up to about 2.  The test asserts 4 x this, the surface tests' margin over
# theirs.
MEASURED_COLOUR = 3.4e-6
LEFT_OUT = 0.02   # the share of a case's pixels the comparison may leave out because a fetch picked other texels


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: ref.render(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


@pytest.fixture(scope="module")
def twins(scenes):
    return {name: ref.render(s, twin=True) for name, s in scenes.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_reaches_what_it_was_built_for(scenes, rendered, name):
    assert cases.CASES[name][1](rendered[name], scenes[name]), rendered[name]["stats"]


def test_the_frames_hold_two_whole_bins_and_a_partial_one_on_each_axis():
    assert cases.W > 2 * ref.BIN and cases.W % ref.BIN and cases.H > 2 * ref.BIN and cases.H % ref.BIN
    assert cases.NUM_SOUPS == 20


def test_golden_file(rendered):
    assert GOLDEN.stat().st_size < 32 * 1024
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        r = ref.render(golden_scene(g, name))
        assert ref.same_bits_or_class(r["target"], g[f"{name}.target"]).all(), name
        assert ref.same_bits_or_class(rendered[name]["target"], g[f"{name}.target"]).all(), f"{name}: the case no longer is what the file holds"


def test_a_band_is_the_rows_of_the_whole_frame(scenes, rendered):
    for name, s in scenes.items():
        r0, r1 = s["rows"]
        assert (r0, r1) != (0, s["H"])
        band, whole = ref.render(s, rows=(r0, r1)), rendered[name]
        np.testing.assert_array_equal(band["count"], whole["count"][r0:r1], err_msg=name)
        assert ref.same_bits_or_class(band["target"], whole["target"][r0:r1]).all(), name


def test_restatement_against_its_float64_twin(scenes, rendered, twins):
    worst, worst_name = 0.0, ""
    for name, r in rendered.items():
        t = twins[name]
        np.testing.assert_array_equal(r["count"], t["count"], err_msg=f"{name}: coverage and scissor ownership are exact for both, no pixel left out")
        np.testing.assert_array_equal(r["last"], t["last"], err_msg=name)
        out = np.zeros(r["count"].shape, bool)
        assert len(r["taps"]) == len(t["taps"])
        for (k, j, i, x0, y0), (k2, j2, i2, x2, y2) in zip(r["taps"], t["taps"]):
            assert k == k2 and np.array_equal(j, j2) and np.array_equal(i, i2)
            other = (x0 != x2) | (y0 != y2)
            out[j[other], i[other]] = True
        share = out.mean()
        assert share <= LEFT_OUT, f"{name}: {share:.2%} of the pixels fetch other texels in float64"
        a, b = r["target"].astype(np.float64), t["target"]
        finite = np.isfinite(a) & np.isfinite(b) & ~out[..., None]
        assert ((np.isnan(a) == np.isnan(b)) | out[..., None]).all(), name
        with np.errstate(all="ignore"):
            d = float(np.abs(a - b)[finite].max()) if finite.any() else 0.0
        if d > worst:
            worst, worst_name = d, name
    print(f"max |c32 - c64| = {worst:.3e} ({worst_name})")
    assert worst <= 4 * MEASURED_COLOUR, (worst, worst_name)
    assert worst >= MEASURED_COLOUR / 2, "the recorded figure is far above the worst measured: measure again and update DESIGN.md"


def test_the_reverse_order_mutant_differs(scenes, rendered):
    told = []
    for name in ("order_abc", "chunk_seam_257", "chunk_seam_513", "aa_fringe", "soup_0"):
        m = ref.render(scenes[name], reverse=True)
        np.testing.assert_array_equal(m["count"], rendered[name]["count"])   # order does not decide coverage
        if not ref.same_bits_or_class(m["target"], rendered[name]["target"]).all():
            told.append(name)
    assert "order_abc" in told and "chunk_seam_257" in told and "chunk_seam_513" in told, told
    # ... and the two orders of the same three rects give different bits
    assert not ref.same_bits_or_class(rendered["order_abc"]["target"], rendered["order_cba"]["target"]).all()
    # a single rect has no order to get wrong: its two triangles share no pixel
    one = ref.render(scenes["shared_diagonal"], reverse=True)
    assert ref.same_bits_or_class(one["target"], rendered["shared_diagonal"]["target"]).all()


def test_known_answers_by_hand():
    # half-transparent red over (0.25, 0.5, 0.75, 0.75): rgb = 1 * 0.5 + dst * 0.5 with 128 / 255 for the alpha byte; a = sa * sa - 0.75 * (1 - sa)
    l = cases.dl().clip(0, 0, 8, 8).rect(2, 2, 6, 6, cases.HALF_RED)
    t = np.zeros((8, 8, 4), np.float32)
    t[:] = (0.25, 0.5, 0.75, 0.75)
    s = cases.scene([l], target=t, display_size=(8, 8), w=8, h=8, rows=(1, 5))
    r = ref.render(s)
    sa = np.float32(128) / np.float32(255)
    om = np.float32(1) - sa
    # (the rect's area is a power of two, so the l_k are exact and the interpolated colour is the vertices'; src = colour * the white texel)
    want = np.float32([np.float32(1) * sa + np.float32(0.25) * om, np.float32(0) * sa + np.float32(0.5) * om, np.float32(0) * sa + np.float32(0.75) * om,
                       sa * sa - np.float32(0.75) * om])
    assert (r["count"][2:6, 2:6] == 1).all() and r["count"].sum() == 16
    np.testing.assert_array_equal(r["target"][3, 3], want)
    np.testing.assert_array_equal(r["target"][0, 0], t[0, 0])


def _c_flatten(draw_data):
    from sailor_amd import host
    return host.ui_flatten(draw_data)


def _draw_datas():
    from sailor_amd.host import ui_draw_data
    rng = np.random.default_rng(11)
    out = []
    for k in range(40):
        pos = (0.0, 0.0) if k % 3 == 0 else tuple(rng.uniform(-50, 150, 2))
        fbs = [(1.0, 1.0), (2.0, 2.0), (1.5, 1.25)][k % 3]
        size = tuple(rng.uniform(20, 200, 2))
        lists = []
        for _ in range(int(rng.integers(0, 4))):
            l = cases.dl()
            for _ in range(int(rng.integers(0, 6))):
                kind = rng.random()
                if kind < 0.15:
                    l.callback(ref.CALLBACK_RESET if kind < 0.07 else ref.CALLBACK_USER)
                    continue
                x0, y0 = pos[0] + rng.uniform(-30, size[0]), pos[1] + rng.uniform(-30, size[1])
                w, h = rng.choice([-3.0, 0.0, 0.4, 0.9, 5.5, 80.0, 1000.0], 2)
                l.clip(x0, y0, x0 + w, y0 + h).rect(x0, y0, x0 + 9, y0 + 9, cases.HALF_RED)
                if rng.random() < 0.3:
                    l.rect(x0, y0, x0 + 3, y0 + 3, cases.HALF_BLUE)
            lists.append(l)
        out.append(ui_draw_data(lists, size, pos, fbs))
    out.append(ui_draw_data([cases.dl().clip(0, 0, 5, 5).rect(0, 0, 5, 5, cases.HALF_RED)], (0.5, 100.0)))            # (int)(0.5 * 1) == 0: nothing
    out.append(ui_draw_data([cases.dl().clip(0, 0, 5, 5).rect(0, 0, 5, 5, cases.HALF_RED)], (100.0, 3.0), (0, 0), (1.0, 0.3)))   # (int)(0.9) == 0
    out.append(ui_draw_data([cases.dl().clip(float("nan"), 0, 5, 5).rect(0, 0, 5, 5, cases.HALF_RED)], (64.0, 64.0)))  # a NaN ClipRect is left out
    return out


def test_host_flatten_against_the_python_restatement(scenes):
    datas = _draw_datas()
    skipped = kept = 0
    for d in datas:
        want, got = ref.flatten(d), _c_flatten(d)
        assert (got["width"], got["height"]) == (want["width"], want["height"])
        np.testing.assert_array_equal(got["scale"].view(np.uint32), want["scale"].view(np.uint32))
        np.testing.assert_array_equal(got["translate"].view(np.uint32), want["translate"].view(np.uint32))
        assert got["commands"].tobytes() == want["commands"].astype(ref.COMMAND).tobytes(), (got["commands"], want["commands"])
        assert got["vertices"].tobytes() == want["vertices"].tobytes() and np.array_equal(got["indices"], want["indices"])
        n = sum(1 for l in d["lists"] for c in l["cmds"])
        kept += len(want["commands"]); skipped += n - len(want["commands"])
    assert kept > 30 and skipped > 30, (kept, skipped)
    assert len(ref.flatten(datas[-3])["commands"]) == len(ref.flatten(datas[-2])["commands"]) == len(ref.flatten(datas[-1])["commands"]) == 0
    # every clamp of :240-243 and the truncated difference of :251, by hand
    from sailor_amd.host import ui_draw_data
    d = ui_draw_data([cases.dl().clip(-4, -7, 500, 600).clip(3.7, 2.2, 9.2, 30.9).clip(70.5, 60.5, 80, 90)], (72.0, 70.0))
    for c in d["lists"][0]["cmds"]:
        c["elem_count"] = 3
    np.testing.assert_array_equal(_c_flatten(d)["commands"]["scissor"], [[0, 0, 72, 70], [3, 2, 5, 28], [70, 60, 1, 9]])


def test_abi_symbols_struct_sizes_and_null_context_refusals():
    from sailor_amd import _lib
    lib = _lib.load()
    for name in ("sailor_hip_ui_workspace_bytes", "sailor_hip_ui_draw", "sailor_host_ui_flatten"):
        assert hasattr(lib, name)
    assert C.sizeof(_lib.UiCommand) == 28 == np.dtype(_lib.UI_COMMAND_DTYPE).itemsize == ref.COMMAND.itemsize
    assert np.dtype(_lib.VERTEX_P2UV2C1_DTYPE).itemsize == 20 == ref.VERTEX.itemsize
    assert C.sizeof(_lib.UiDrawCmd) == 32 and C.sizeof(_lib.UiDrawList) == 16
    n = C.c_size_t(7)
    assert lib.sailor_hip_ui_workspace_bytes(10, 0, 40, C.byref(n)) == -1 and n.value == 0
    assert lib.sailor_hip_ui_workspace_bytes(10, 72, 40, C.byref(n)) == 0 and n.value >= 10 * 80
    small = n.value
    assert lib.sailor_hip_ui_workspace_bytes(1000, 72, 40, C.byref(n)) == 0 and n.value == small + 990 * 80
    assert lib.sailor_hip_ui_draw(None, None, 0, None, 2, 0, None, None, 0, None, None, None, None, 0, None, 72, 40, None) == -1


def test_the_node_is_registered_and_the_shipped_frame_names_it_last():
    from sailor_amd import runtime_binding
    rt = runtime_binding.load()
    assert rt.sailor_rt_node_registered(b"RenderImGui") == 1   # FrameGraph/RenderImGuiNode.cpp
    assert hasattr(rt, "sailor_rt_set_ui_draw_data")
    text = (Path(__file__).resolve().parent / "golden" / "DefaultRenderer.renderer").read_text()
    _, summary = runtime_binding.parse_renderer(text, 3840, 2160)
    nodes = summary[summary.index("nodes="):summary.index(";values=")]
    entry = "RenderImGui[]{rt color=BackBuffer;rt depthStencil=DepthBuffer;}"
    assert nodes.rstrip(";").endswith(entry) or nodes.endswith(entry), nodes
