"""The surface pass without a GPU: tests/surface_ref.py (the sequential float32 restatement the kernels of sailor_amd/csrc/surface.hip are held to) against the
project's own depth oracle, against closed forms computed in float64 here, against the counts every case of tests/surface_cases.py was built to reach, and
against the golden file; sailor_host_srgb_table against the double formula."""
import math
from pathlib import Path

import numpy as np
import pytest

import surface_cases as cases
import surface_ref as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "tiny_surface.npz"
# The worst errors of the float32 restatement against the float64 closed forms below (measured, and recorded in DESIGN.md 4, "RenderScene: the surface
# pass"); the tests assert 4 x these: headroom for a different but legal rounding order in a second restatement.
#   world    : |worldPos - unprojected pixel centre| on the constant-material quad.  Not a rounding figure: the vertices are snapped to 1 / 256 pixel before
#              the edge functions are taken, so the position belongs to a triangle moved by up to 1 / 512 pixel (a pixel is 0.25 world units there)
#   material : the other nine channels of that quad, relative with a floor of 1
#   uv       : |uv - worldPos.xy| on the oblique quad
#   oblique  : |worldPos - the pixel's ray through the owning triangle's plane| on the oblique quad (snapping again, at up to 9 units from the eye)
MEASURED = dict(world=2.48e-4, material=1.27e-7, uv=2.39e-7, oblique=1.08e-3)


@pytest.fixture(scope="module")
def rendered():
    return {name: ref.render(build()) for name, (build, _) in cases.CASES.items()}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_depth_is_the_depth_oracles_bit_for_bit_with_and_without_a_prepass(rendered, name):
    s = cases.CASES[name][0]()
    want = cases.prepass_depth(s)
    got = rendered[name]
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(got["covered"], want > 0)
    behind = ref.render(s, prepass=want)   # every fragment that won without a prepass ties with it and wins again
    for k in ("depth", "covered", "keys"):
        np.testing.assert_array_equal(behind[k], got[k])
    assert ref.same_bits_or_class(behind["planes"], got["planes"]).all()


def test_depth_with_back_face_culling():
    fewer = 0
    for name in cases.CULL_BACK_CASES:
        s = cases.with_cull_back(cases.CASES[name][0]())
        got, plain = ref.render(s), ref.render(cases.CASES[name][0]())
        np.testing.assert_array_equal(got["depth"].view(np.uint32), cases.prepass_depth(s).view(np.uint32))
        assert got["stats"]["fragments"] <= plain["stats"]["fragments"]
        fewer += got["stats"]["fragments"] < plain["stats"]["fragments"]
    assert fewer >= 3, "back-face culling removes nothing from these cases"


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_reaches_what_it_was_built_for(rendered, name):
    assert cases.CASES[name][1](rendered[name]), rendered[name]["stats"]


def test_random_soups_reach_cuts_ties_and_the_sampler_beyond_the_table():
    total = dict(cut_one=0, cut_two=0, beyond_table=0, overwritten=0, degenerate=0)
    for seed in range(0, cases.NUM_SOUPS, 5):
        st = ref.render(cases.random_soup(seed))["stats"]
        for k in total:
            total[k] += st[k]
    assert all(v > 0 for v in total.values()), total


def test_shared_edges_cover_every_pixel_exactly_once(rendered):
    for name in ("shared_edge_quad", "fan_around_a_pixel_centre"):
        r = rendered[name]
        assert r["stats"]["overwritten"] == 0 and r["stats"]["fragments"] == r["covered"].sum() > 100, (name, r["stats"])


def test_a_prepass_with_geometry_the_scene_does_not_draw_keeps_its_depth_uncovered():
    for name in ("multiple_draws", "near_plane"):
        s = cases.CASES[name][0]()
        own, both = cases.prepass_depth(s), cases.prepass_depth(s, cases.prepass_only_draw(s))
        hidden = both != own
        assert hidden.sum() > 20
        r = ref.render(s, prepass=both)
        assert not r["covered"][hidden].any()
        np.testing.assert_array_equal(r["depth"].view(np.uint32), both.view(np.uint32))
        for k in range(3):
            assert (r["planes"][k][hidden] == ref.UNCOVERED[k]).all()
        plain = ref.render(s)
        assert ref.same_bits_or_class(r["planes"][:, ~hidden], plain["planes"][:, ~hidden]).all()


def test_bands_concatenate_to_the_whole_frame(rendered):
    for name in cases.BAND_CASES:
        s, whole = cases.CASES[name][0](), rendered[name]
        H = s["H"]
        tile_rows = -(-H // 16)
        for world in (2, 3):
            # framebuffer rows of the bands of `world` ranks: rank r holds tile rows r T / world .. (r + 1) T / world, and tile row t = rows
            # H - 16 (t + 1) .. H - 16 t, the topmost cut at row 0 (72 x 40: 0 / 24 / 40 and 0 / 8 / 24 / 40; 200 x 136: 0 / 72 / 136 and 0 / 40 / 88 / 136)
            bounds = sorted(max(0, H - 16 * (r * tile_rows // world)) for r in range(world + 1))
            parts = [ref.render(s, rows=(a, b)) for a, b in zip(bounds[:-1], bounds[1:])]
            np.testing.assert_array_equal(np.concatenate([p["keys"] for p in parts]), whole["keys"])
            assert ref.same_bits_or_class(np.concatenate([p["planes"] for p in parts], axis=1), whole["planes"]).all()


# ---- closed forms, in float64 ---------------------------------------------------------------------------------------------------------------------
def _unproject(s, i, j, plane_point, plane_normal):
    """the point where the ray of pixel centre (i + 0.5, j + 0.5) meets the plane, float64 (view = identity, eye at the origin)"""
    P = np.asarray(s["projection"], np.float64).reshape(4, 4).T
    nx, ny = (i + 0.5) / (s["W"] * 0.5) - 1.0, 1.0 - (j + 0.5) / (s["H"] * 0.5)
    ray = np.array([nx / P[0, 0], ny / P[1, 1], -1.0])
    return ray * (plane_point @ plane_normal) / (ray @ plane_normal)


def _srgb(b):
    c = b / 255.0
    return c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4)


def _worst_errors(perspective):
    s = cases.constant_material_quad()
    r = ref.render(s, perspective=perspective)
    M = np.asarray(s["instances"]["model"][0], np.float64).reshape(4, 4).T
    m = s["materials"][0]
    a, n = s["textures"][0][0, 0].astype(np.float64), s["textures"][1][0, 0].astype(np.float64)
    colour = np.array([0.8, 0.7, 0.6, 0.9], np.float32).astype(np.float64)
    texel = np.array([_srgb(a[0]), _srgb(a[1]), _srgb(a[2]), a[3] / 255.0])
    albedo = m["albedo"].astype(np.float64) * texel * colour
    tn = 2.0 * n[:3] / 255.0 - 1.0
    tn /= np.linalg.norm(tn)
    wn = M[:3, :3] @ tn   # tangent, bitangent, normal are the unit axes: TBN = mat3(model)
    wn /= np.linalg.norm(wn)
    point, normal = M[:3, 3] + M[:3, :3] @ np.array([0, 0, -3.0]), M[:3, :3] @ np.array([0, 0, 1.0])
    assert r["covered"].all()
    world = material = 0.0
    for j in range(s["H"]):
        for i in range(s["W"]):
            got = r["planes"][:, j, i].reshape(12).astype(np.float64)
            world = max(world, float(np.max(np.abs(got[0:3] - _unproject(s, i, j, point, normal)))))
            want = np.concatenate([[albedo[3]], wn, [float(m["roughness"]) * texel[0]], albedo[:3], [float(m["metallic"]) * texel[0]]])
            material = max(material, float(np.max(np.abs(got[3:] - want) / np.maximum(np.abs(want), 1.0))))
    # uv is not an output: the oblique quad is rendered with its texcoord as vertex colour too, which comes out in P2 (albedo = 1 * 1 * colour)
    so = cases.oblique_quad()
    so["draws"][0]["vertices"][:, 14:16] = so["draws"][0]["vertices"][:, 0:2]
    o = ref.render(so, perspective=perspective)
    c = o["covered"]
    assert c.sum() > 150
    uv = float(np.max(np.abs(o["planes"][2][c][:, 0:2].astype(np.float64) - o["planes"][0][c][:, 0:2].astype(np.float64))))
    # ... and its world position against the pixel's ray through the plane of the triangle that owns the pixel (the mutant keeps uv == worldPos.xy: both go wrong alike)
    Mo = np.asarray(so["instances"]["model"][0], np.float64).reshape(4, 4).T
    verts = [(Mo @ np.array([*v[2:5].astype(np.float64), 1.0]))[:3] for v in so["draws"][0]["vertices"]]
    oblique = 0.0
    for j, i in zip(*np.nonzero(c)):
        t = so["draws"][0]["indices"][(int(o["keys"][j, i] & np.uint64(0xFFFFFFFF)) - 1) >> 1]
        nrm = np.cross(verts[t[1]] - verts[t[0]], verts[t[2]] - verts[t[0]])
        oblique = max(oblique, float(np.max(np.abs(o["planes"][0][j, i, 0:3] - _unproject(so, i, j, verts[t[0]], nrm)))))
    return dict(world=world, material=material, uv=uv, oblique=oblique)


def test_known_answers_in_closed_form_and_the_screen_linear_mutant_breaks_them():
    got = _worst_errors(True)
    print("restatement against the float64 closed forms:", {k: f"{v:.3e}" for k, v in got.items()})
    for k, v in got.items():
        assert v <= 4 * MEASURED[k], (k, v)
        assert v >= MEASURED[k] / 2, f"the recorded figure of {k} is far above the worst measured: measure again and update DESIGN.md"
    mutant = _worst_errors(False)
    print("the screen-linear mutant:", {k: f"{v:.3e}" for k, v in mutant.items()})
    assert mutant["oblique"] > 100 * 4 * MEASURED["oblique"], "a non-perspective interpolation passes: the cases do not test it"


def test_srgb_table_is_the_double_formula_rounded_once():
    from sailor_amd import host
    want = np.array([_srgb(i) for i in range(256)], np.float64).astype(np.float32)
    np.testing.assert_array_equal(host.srgb_table().view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(ref.srgb_table().view(np.uint32), want.view(np.uint32))
    assert want[0] == 0 and want[255] == 1 and (np.diff(want) > 0).all()


def test_draw_prims_and_struct_sizes():
    from sailor_amd import _lib, host
    assert host.surface_draw_prims(12, 1024) == 24576 and host.surface_draw_prims(0xFFFFFFFF, 0xFFFFFFFF) == 2 ** 64 - 1   # saturates
    assert np.dtype(_lib.VERTEX_DTYPE).itemsize == 72 and np.dtype(_lib.MATERIAL_DTYPE).itemsize == 80 and host.INSTANCE_DTYPE.itemsize == 96


def test_golden_file_against_the_restatement():
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        r = ref.render(cases.scene_from_arrays(g, name))   # the scene as the file holds it
        np.testing.assert_array_equal(g[f"{name}.keys"], r["keys"])
        assert ref.same_bits_or_class(g[f"{name}.planes"], r["planes"]).all()
        now = cases.scene_to_arrays(cases.CASES[name][0](), name)   # ... and the case has not drifted from it
        assert set(now) == {k for k in g.files if k.startswith(name + ".")} - {f"{name}.keys", f"{name}.planes"}
        for k, v in now.items():
            np.testing.assert_array_equal(g[k].view(np.uint8), np.ascontiguousarray(v).view(np.uint8), err_msg=k)
