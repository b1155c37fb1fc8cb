"""The DebugDraw pass without a GPU: tests/lines_ref.py (the sequential float32 restatement the kernels of sailor_amd/csrc/debug_lines.hip are held to) against
what every case of tests/lines_cases.py was built to reach, against its float64 twin (coverage and owners equal, z and colour within 4 x the measured error),
against its screen-linear mutant, against answers worked out by hand, and against the golden file; the host helpers of sailor_amd/host.py against closed forms;
the C-ABI's symbols, struct sizes and NULL-context refusals."""
import ctypes as C

import numpy as np
import pytest

import lines_cases as cases
import lines_ref as ref
from make_lines_golden import PATH as GOLDEN, golden_scene

# the largest |fp32 - float64| over every owned pixel of every case and soup, as measured (recorded in DESIGN.md, "DebugDraw"); the bounds are 4 x these, the
# project's convention: headroom for a different but legal rounding order
MEASURED_Z_ERROR = 1.15e-6
MEASURED_COLOUR_ERROR = 2.13e-7
Z_BOUND, COLOUR_BOUND = 4 * MEASURED_Z_ERROR, 4 * MEASURED_COLOUR_ERROR


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: ref.render(s) for name, s in scenes.items()}


@pytest.fixture(scope="module")
def twins(scenes):
    return {name: ref.render(s, twin=True) for name, s in scenes.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_reaches_what_it_was_built_for(scenes, rendered, name):
    assert cases.CASES[name][1](rendered[name], scenes[name]), rendered[name]["stats"]


def test_every_branch_is_reached_by_some_case(rendered):
    total = {}
    for r in rendered.values():
        for k, v in r["stats"].items():
            total[k] = total.get(k, 0) + v
    assert [b for b in cases.BRANCHES if total.get(b, 0) == 0] == [], total
    assert set(total) <= set(cases.BRANCHES), set(total) - set(cases.BRANCHES)   # nothing is counted that the list does not name
    named = {}
    for name in cases.CASES:   # ... and the named cases alone reach them too, without the soups
        for k, v in rendered[name]["stats"].items():
            named[k] = named.get(k, 0) + v
    assert [b for b in cases.BRANCHES if named.get(b, 0) == 0] == [], named


def test_a_band_is_the_rows_of_the_whole_frame(scenes, rendered):
    for name, s in scenes.items():
        r0, r1 = s["rows"]
        assert (r0, r1) != (0, s["H"])
        band, whole = ref.render(s, rows=(r0, r1)), rendered[name]
        np.testing.assert_array_equal(band["keys"], whole["keys"][r0:r1], err_msg=name)
        assert ref.same_bits_or_class(band["target"], whole["target"][r0:r1]).all(), name
        np.testing.assert_array_equal(band["depth"][r0:r1].view(np.uint32), whole["depth"][r0:r1].view(np.uint32), err_msg=name)
        seed = np.zeros_like(band["depth"]) if s["depth"] is None else s["depth"]
        np.testing.assert_array_equal(np.delete(band["depth"], np.s_[r0:r1], 0), np.delete(seed, np.s_[r0:r1], 0), err_msg=f"{name}: depth outside the band")


def errors(a, b, owner):
    m = owner >= 0
    z = np.abs(a["depth"][a["rows"][0]:a["rows"][1]][m].astype(np.float64) - b["depth"][b["rows"][0]:b["rows"][1]][m])
    c = np.abs(a["target"][m].astype(np.float64) - b["target"][m])
    c = c[np.isfinite(c)]
    return (float(z.max()) if z.size else 0.0), (float(c.max()) if c.size else 0.0), int(m.sum())


def test_restatement_against_its_float64_twin(rendered, twins):
    worst_z = worst_c = 0.0
    pixels = 0
    for name, r in rendered.items():
        t = twins[name]
        np.testing.assert_array_equal(r["owner"], t["owner"], err_msg=f"{name}: coverage and owners are exact for both, no case left out")
        assert {k: v for k, v in r["stats"].items()} == {k: v for k, v in t["stats"].items()}, name
        z, c, n = errors(r, t, r["owner"])
        print(f"{name}: {n} owned pixels, max |z32 - z64| = {z:.3g}, max |c32 - c64| = {c:.3g}")
        worst_z, worst_c, pixels = max(worst_z, z), max(worst_c, c), pixels + n
    print(f"over everything: {pixels} owned pixels, max |z32 - z64| = {worst_z:.3g}, max |c32 - c64| = {worst_c:.3g}")
    assert pixels > 4000
    assert worst_z <= Z_BOUND and worst_c <= COLOUR_BOUND, (worst_z, worst_c)


def test_the_screen_linear_mutant_fails_the_colour_bound(scenes, rendered, twins):
    name = "end_colours_with_very_different_w"
    mutant = ref.render(scenes[name], perspective=False)
    np.testing.assert_array_equal(mutant["keys"], rendered[name]["keys"])   # colour does not decide ownership
    z, c, n = errors(mutant, twins[name], mutant["owner"])
    print(f"mutant: {n} owned pixels, max |c32 - c64| = {c:.3g}")
    assert z <= Z_BOUND and c > 1000 * COLOUR_BOUND, (z, c)


def test_known_answers_by_hand():
    # exact 45 degrees from pixel centre (2.5, 2.5) to (6.5, 6.5): |dX| == |dY| is x-major; columns 2..5 (X0 <= 256 c + 128 < X1: start in, end out); the row of
    # column c is floor((640 x 1024 + 1024 (256 c + 128 - 640)) / (256 x 1024)) = c
    s = cases.make_scene(16, 12, [cases.seg((2.5, 2.5), (6.5, 6.5))], (1, 8))
    assert cases.owned(ref.render(s)) == {(2, 2), (3, 3), (4, 4), (5, 5)}
    # ... and back: X1 < M <= X0 gives columns 3..6
    s = cases.make_scene(16, 12, [cases.seg((6.5, 6.5), (2.5, 2.5))], (1, 8))
    assert cases.owned(ref.render(s)) == {(3, 3), (4, 4), (5, 5), (6, 6)}
    # the anti-diagonal from (2.5, 6.5) to (6.5, 2.5): row of column c = floor((1664 x 1024 - 1024 (256 c - 512)) / 262144) = floor((2176 - 256 c) / 256) = 8 - c
    s = cases.make_scene(16, 12, [cases.seg((2.5, 6.5), (6.5, 2.5))], (1, 8))
    assert cases.owned(ref.render(s)) == {(2, 6), (3, 5), (4, 4), (5, 3)}
    # slope 1/2 from the pixel corner (2, 2) to (8, 5): centres 2.5 .. 7.5, y = 2 + (x - 2) / 2 = 2.25, 2.75, 3.25, 3.75, 4.25, 4.75
    s = cases.make_scene(16, 12, [cases.seg((2.0, 2.0), (8.0, 5.0))], (1, 8))
    assert cases.owned(ref.render(s)) == {(2, 2), (3, 2), (4, 3), (5, 3), (6, 4), (7, 4)}
    # the floor tie: y = 3 exactly on a row border belongs to row 3; the same segment a 256th higher to row 2
    s = cases.make_scene(16, 12, [cases.seg((2.0, 3.0), (4.0, 3.0))], (1, 8))
    assert cases.owned(ref.render(s)) == {(2, 3), (3, 3)}
    s = cases.make_scene(16, 12, [cases.seg((2.0, 3.0 - 1 / 256), (4.0, 3.0 - 1 / 256))], (1, 8))
    assert cases.owned(ref.render(s)) == {(2, 2), (3, 2)}
    # depth tie of two segments: the later one owns the crossing; colour at the middle of a w = 1 segment is the mean
    s = cases.make_scene(16, 12, [cases.seg((2.5, 4.5), (10.5, 4.5), (1, 0, 0, 1), (0, 0, 1, 0)), cases.seg((6.5, 1.5), (6.5, 8.5), (0, 1, 0, 1))], (1, 8))
    r = ref.render(s)
    assert r["owner"][4, 6] == 1 and r["owner"][4, 5] == 0 and r["keys"][4, 6] == (np.uint64(np.float32(0.5).view(np.uint32)) << np.uint64(32)) | np.uint64(2)
    np.testing.assert_array_equal(r["target"][4, 5], np.float32([1 - 3 / 8, 0, 3 / 8, 1 - 3 / 8]))
    np.testing.assert_array_equal(r["target"][4, 6], np.float32([0, 1, 0, 1]))
    np.testing.assert_array_equal(r["target"][0, 0], s["target"][0, 0])   # an unowned pixel keeps Main


def test_host_helpers_against_closed_forms():
    from sailor_amd import host
    lo, hi = np.float32([-1, 2, 3]), np.float32([4, 5, 7])
    v = host.debug_aabb(lo, hi, (1, 0.5, 0.25, 1))
    assert len(v) == 24 and (v["color"] == np.float32([1, 0.5, 0.25, 1])).all()
    p = v["position"].reshape(12, 2, 3)
    c = lambda x, y, z: [(lo, hi)[x][0], (lo, hi)[y][1], (lo, hi)[z][2]]  # noqa: E731
    want = [(c(0, 0, 0), c(1, 0, 0)), (c(0, 0, 0), c(0, 1, 0)), (c(0, 0, 0), c(0, 0, 1)), (c(1, 1, 1), c(0, 1, 1)), (c(1, 1, 1), c(1, 0, 1)), (c(1, 1, 1), c(1, 1, 0)),
            (c(0, 1, 1), c(0, 1, 0)), (c(0, 1, 1), c(0, 0, 1)), (c(0, 0, 1), c(1, 0, 1)), (c(1, 0, 1), c(1, 0, 0)), (c(1, 0, 0), c(1, 1, 0)), (c(1, 1, 0), c(0, 1, 0))]
    np.testing.assert_array_equal(p, np.float32(want))   # DebugContext.cpp:102-115, in order
    # every edge of the box once: 12 distinct unordered pairs that differ in exactly one coordinate
    edges = {frozenset((tuple(a), tuple(b))) for a, b in p}
    assert len(edges) == 12 and all((a != b).sum() == 1 for a, b in p)

    s = host.debug_sphere([1, 2, 3], 2.0, (1, 1, 1, 1))
    assert len(s) == 2 * 8 * (1 + 7 * 3)   # DrawSphere: 8 latitude bands, the first longitude one segment, the other seven three
    d = np.linalg.norm(s["position"].astype(np.float64) - [1, 2, 3], axis=1)
    assert np.abs(d - 2.0).max() < 1e-5      # every vertex on the sphere
    q = s["position"].reshape(-1, 2, 3)
    # the (i - 1) indexing: the first band starts below the pole, lat0 = pi (-0.5 - 1/7); the (j - 1): the first meridian is at -2 pi / 7
    pi = np.float32(3.1415926)
    lat0, lng0 = pi * (np.float32(-0.5) + np.float32(-1) / np.float32(7)), np.float32(2) * pi * np.float32(-1) / np.float32(7)
    np.testing.assert_allclose(q[0][0], [1 + 2 * np.cos(lng0) * np.cos(lat0), 2 + 2 * np.sin(lat0), 3 + 2 * np.sin(lng0) * np.cos(lat0)], rtol=0, atol=1e-6)

    corners = np.float32([[i, j, k] for k in (0, 1) for j in (0, 1) for i in (0, 1)])
    f = host.debug_frustum(corners, (1, 0, 0, 1))
    assert len(f) == 24 and (f["color"].reshape(12, 2, 4)[4:8] == 1).all() and (f["color"].reshape(12, 2, 4)[:4] == np.float32([1, 0, 0, 1])).all()
    np.testing.assert_array_equal(f["position"].reshape(12, 2, 3)[8], [corners[4], corners[0]])

    m = np.float32([[0, 2, 0, 0], [-2, 0, 0, 0], [0, 0, 2, 0], [5, 5, 5, 1]])   # columns: a rotation about z with scale 2, and a translation the axes ignore (w = 0)
    o = host.debug_origin([1, 1, 1], m, 3.0)
    np.testing.assert_array_equal(o["position"], np.float32([[1, 1, 1], [1, 7, 1], [1, 1, 1], [-5, 1, 1], [1, 1, 1], [1, 1, 7]]))
    np.testing.assert_array_equal(o["color"][::2], np.float32([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1]]))

    a = host.debug_arrow([0, 0, 0], [0, 3, 4], (1, 1, 1, 1))   # length 5: the cross has half-width 0.5
    assert len(a) == 8
    np.testing.assert_allclose(a["position"], [[0, 0, 0], [0, 3, 4], [0, 3.5, 4], [0, 2.5, 4], [-0.5, 3, 4], [0.5, 3, 4], [0, 3, 3.5], [0, 3, 4.5]], rtol=0, atol=1e-6)
    line = host.debug_line([1, 2, 3], [4, 5, 6], (0.1, 0.2, 0.3, 0.4))
    assert line.dtype.itemsize == 28 and line.tobytes() == np.float32([1, 2, 3, 0.1, 0.2, 0.3, 0.4, 4, 5, 6, 0.1, 0.2, 0.3, 0.4]).tobytes()


def test_abi_symbols_struct_sizes_and_null_context_refusals():
    from sailor_amd import _lib, host
    try:
        lib = _lib.load()
    except OSError as e:
        pytest.skip(f"libsailor_hip.so does not load here: {e}")
    for name in ("sailor_hip_debug_lines_draw", "sailor_hip_debug_lines_resolve", "sailor_hip_debug_lines_prims"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert C.sizeof(_lib.DebugLinesDraw) == 24 and np.dtype(_lib.VERTEX_P3C4_DTYPE).itemsize == 28 == ref.VERTEX.itemsize
    assert host.debug_lines_prims(0) == 0 and host.debug_lines_prims(12) == 12 and host.debug_lines_prims(0xFFFFFFFF) == 0xFFFFFFFF
    assert lib.sailor_hip_debug_lines_prims(3, None) == -1
    d = _lib.DebugLinesDraw(None, None, 0, 0)
    vp = (C.c_float * 16)()
    band = host.band_whole_frame(16, 12)
    assert lib.sailor_hip_debug_lines_draw(None, vp, C.byref(d), 16, 12, C.byref(band), None, 0) == -1
    assert lib.sailor_hip_debug_lines_resolve(None, vp, C.byref(d), 16, 12, C.byref(band), None, 0, None, None) == -1


def test_the_debug_draw_node_is_registered_and_the_shipped_frame_names_it_behind_render_scene():
    from pathlib import Path
    from sailor_amd import runtime_binding
    rt = runtime_binding.load()
    assert rt.sailor_rt_node_registered(b"DebugDraw") == 1   # FrameGraph/DebugDrawNode.cpp:16
    for name in ("line", "aabb", "frustum", "origin", "sphere"):
        assert hasattr(rt, f"sailor_rt_debug_draw_{name}")
    assert hasattr(rt, "sailor_rt_debug_tick") and rt.sailor_rt_debug_tick(None, 0.1) == -1
    text = (Path(__file__).resolve().parent / "golden" / "DefaultRenderer.renderer").read_text()
    _, summary = runtime_binding.parse_renderer(text, 3840, 2160)
    nodes = summary[summary.index("nodes="):summary.index(";values=")]
    entry = "DebugDraw[]{rt color=Main;rt depthStencil=DepthBuffer;}"
    assert entry in nodes and nodes.rindex("RenderScene[") < nodes.index(entry) < nodes.index("Bloom["), nodes


def test_golden_file():
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        r = ref.render(golden_scene(g, name))
        np.testing.assert_array_equal(r["keys"], g[f"{name}.keys"])
        assert ref.same_bits_or_class(r["target"], g[f"{name}.target"]).all()
        np.testing.assert_array_equal(r["depth"].view(np.uint32), g[f"{name}.depth_out"].view(np.uint32))
        assert (r["keys"].astype(np.uint32) != 0).sum() > 10
    assert GOLDEN.stat().st_size < 32 * 1024
