"""The multisampled surface pass (sailor_amd/csrc/surface_msaa.hip) without a GPU: the C-ABI's symbols, signatures, version, store size and sample table; the
restatement (tests/msaa_ref.py) held at one sample against tests/surface_ref.py, which the project already trusts; known answers worked by hand; the partition
of closed meshes among their triangles sample by sample; what the cases of tests/msaa_cases.py reach, asserted from the restatement alone; layers, weights and
the accumulate; and every host-side refusal in the stand-alone scripts/msaa_host_check.cpp, which a test here builds with the host sanitizers and runs."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import msaa_cases as cases
import msaa_ref as mr
import surface_cases
import surface_ref
from sailor_amd import _lib, host

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
ENTRIES = ("sailor_host_msaa_sample_positions", "sailor_hip_surface_msaa_bytes", "sailor_hip_surface_msaa_begin", "sailor_hip_surface_msaa_draw",
           "sailor_hip_surface_msaa_draw_gltf", "sailor_hip_surface_msaa_layer", "sailor_hip_surface_msaa_accumulate", "sailor_hip_surface_msaa_store_depth")
# rule 1 of the header's section, restated here once: the tests below read the table from the library
RULE_1 = {1: [(128, 128)], 2: [(192, 192), (64, 64)], 4: [(96, 32), (224, 96), (32, 160), (160, 224)],
          8: [(144, 80), (112, 176), (208, 144), (80, 48), (48, 208), (16, 112), (176, 240), (240, 16)]}
LOW = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def P8():
    return host.msaa_sample_positions(8)


@pytest.fixture(scope="module")
def rendered8(P8):
    """every case at eight samples: computed once, shared, left unchanged"""
    return {name: (s, mr.render(s, P8)) for name, s in ((n, b()) for n, b in cases.CASES.items())}


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_signatures_version_store_size_and_sample_table():
    lib = _lib.load()
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    assert lib.sailor_hip_version() >= 14
    for name in ENTRIES:
        kind = "size_t" if name.endswith("_bytes") else "int"
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"SAILOR_HIP_API {kind} {name}(" in header, name
        declared = re.search(rf"{name}\(([^;]*)\);", header).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [2, 3, 10, 17, 17, 15, 11, 9]
    u32, sz, P = C.c_uint32, C.c_size_t, C.c_void_p
    masked = _lib.SIGNATURES["sailor_hip_surface_draw_masked"][1]
    for name in ENTRIES[3:5]:   # _draw_masked's arguments, then the store
        assert _lib.SIGNATURES[name][1] == masked + [P, sz, u32], name
    band = _lib.Band(0, 3, 0, 35)
    for S in (1, 2, 4, 8):
        assert lib.sailor_hip_surface_msaa_bytes(50, band, S) == 35 * 50 * S * 8
    assert lib.sailor_hip_surface_msaa_bytes(3840, _lib.Band(0, 135, 0, 2160), 8) == 3840 * 2160 * 64 == 530841600   # the 531 MB of DESIGN.md
    assert lib.sailor_hip_surface_msaa_bytes(50, _lib.Band(1, 2, 16, 7), 4) == 7 * 50 * 4 * 8                           # the band's rows
    for width, b, S in ((50, None, 8), (0, band, 8), (-1, band, 8), (32769, band, 8), (50, band, 0), (50, band, 3), (50, band, 16), (50, band, 2 ** 32 - 1),
                        (50, _lib.Band(0, 3, 0, 0), 8), (50, _lib.Band(0, 3, 0, -5), 8)):
        assert lib.sailor_hip_surface_msaa_bytes(width, b, S) == 0, (width, S)
    for S, want in RULE_1.items():
        got = host.msaa_sample_positions(S)
        assert got.tolist() == [list(p) for p in want], S
        assert (got % 16 == 0).all() and got.min() >= 16 and got.max() <= 240 and len({tuple(p) for p in got.tolist()}) == S
    for S in (0, 3, 5, 16, 32, 64):
        with pytest.raises(_lib.SailorHipError):
            host.msaa_sample_positions(S)
    # what a NULL context reaches
    assert lib.sailor_hip_surface_msaa_begin(None, 8, 8, band, None, 0, None, 0, 8, None) == -1
    assert lib.sailor_hip_surface_msaa_draw(None, None, None, None, None, 0, None, 0, 0, 8, 8, band, None, 0, None, 0, 8) == -1
    assert lib.sailor_hip_surface_msaa_draw_gltf(None, None, None, None, None, 0, None, 0, 0, 8, 8, band, None, 0, None, 0, 8) == -1
    assert lib.sailor_hip_surface_msaa_layer(None, 8, 8, band, None, 0, None, 0, 8, 8, 0, None, None, None, None) == -1
    assert lib.sailor_hip_surface_msaa_accumulate(None, None, None, None, None, 8, 0, None, 8, 8, band) == -1
    assert lib.sailor_hip_surface_msaa_store_depth(None, None, 0, 8, None, None, 8, 8, band) == -1


def test_the_existing_draws_keep_their_instantiations_and_the_multisampled_draws_are_two_more():
    """read from the sources: the body's mode and the set-up's box default to what they were; only the new unit asks for SURF_DRAW_MSAA"""
    csrc = ROOT / "sailor_amd" / "csrc"
    body, common = (csrc / "surface_masked_body.h").read_text(), (csrc / "surface_common.h").read_text()
    assert "int MODE = SURF_DRAW_MASKED" in body and "SURF_DRAW_MSAA = 3" in body and "template <bool PIXEL_BOX = false>" in common
    users = [p.name for p in csrc.glob("*.hip") if "SURF_DRAW_MSAA" in p.read_text()]
    assert users == ["surface_msaa.hip"]
    assert (csrc / "surface_msaa.hip").read_text().count("SURF_DRAW_MSAA>(") == 2


# ---- one sample: the restatement's walk against the one the project trusts ------------------------------------------------------------------------------
def test_at_one_sample_the_keys_are_the_surface_restatements_on_every_case_and_soup():
    P1 = host.msaa_sample_positions(1)
    scenes = [(name, build()) for name, (build, _) in surface_cases.CASES.items()] + [(f"soup {k}", surface_cases.random_soup(k)) for k in range(surface_cases.NUM_SOUPS)]
    covered = 0
    for name, s in scenes:
        want = surface_ref.render(s)["keys"]
        got = mr.render(s, P1)["store"][..., 0]
        np.testing.assert_array_equal(got, want, err_msg=name)
        covered += int((want & LOW != 0).sum())
    assert covered > 20000
    s = surface_cases.near_plane()   # ... and over a band, and begun from a depth
    np.testing.assert_array_equal(mr.render(s, P1, rows=(13, 31))["store"][..., 0], surface_ref.render(s, rows=(13, 31))["keys"])
    pre = surface_cases.prepass_depth(s, surface_cases.prepass_only_draw(s))
    np.testing.assert_array_equal(mr.render(s, P1, sample_depth=pre[..., None])["store"][..., 0], surface_ref.render(s, prepass=pre)["keys"])


# ---- known answers, worked by hand ------------------------------------------------------------------------------------------------------------------------
def owned(r, j, i):
    return [int(s) for s in np.nonzero(r["store"][j, i] & LOW)[0]]


def test_a_rectangle_edge_through_the_pixel_centre_owns_the_four_samples_to_its_right(rendered8, P8):
    """the left edge at x = 20 + 128/256: of the eight samples of column 20 those with sx > 128 -- 0 (144), 2 (208), 6 (176), 7 (240) -- for every row 3 .. 8"""
    assert [int(p[0]) for p in P8] == [144, 112, 208, 80, 48, 16, 176, 240]
    _, r = rendered8["edge_rect_left_128"]
    for j in range(3, 9):
        assert owned(r, j, 20) == [0, 2, 6, 7], j
        assert owned(r, j, 19) == [] and owned(r, j, 21) == list(range(8))
    assert owned(r, 2, 20) == [] and owned(r, 9, 20) == []


def test_a_sample_on_the_edge_goes_to_the_rectangle_whose_left_edge_it_is(rendered8):
    """the edge at x = 20 + 144/256 runs through sample 0: owned as a left edge (0, 2, 6, 7 again), not as a right edge (1, 3, 4, 5)"""
    for j in range(3, 9):
        assert owned(rendered8["edge_rect_left_144"][1], j, 20) == [0, 2, 6, 7]
        assert owned(rendered8["edge_rect_right_144"][1], j, 20) == [1, 3, 4, 5]
    _, r = rendered8["shared_edge_rects"]   # two rectangles sharing that edge: every sample of the column exactly once
    assert (r["inside_count"][3:9, 10:30] == 1).all()
    for j in range(3, 9):
        orders = (r["store"][j, 20] & LOW).astype(np.int64)
        assert sorted(np.nonzero(orders > 4)[0].tolist()) == [0, 2, 6, 7] and (orders > 0).all()   # the second draw's orders are 5 .. 8


def test_the_resolved_colour_of_the_half_covered_pixel_is_the_stated_average(rendered8):
    s, r = rendered8["edge_rect_left_128"]
    L = mr.layers(r["store"], 8)
    target = cases.constant_target(s, (0.25, 0.5, 0.125, 1.0))
    colour = np.broadcast_to(np.array([1.0, 0.0, 0.5, 1.0], f32), target.shape)
    out = mr.accumulate(target, colour, L["weights"][0], L["uncovered"], 8, 0)
    assert L["weights"][0][5, 20] == 4 and L["uncovered"][5, 20] == 4 and L["weights"][1][5, 19:22].max() == 0
    assert out[5, 20].tolist() == [0.625, 0.25, 0.3125, 1.0]          # 4/8 of each, exact in fp32
    assert out[5, 19].tolist() == [0.25, 0.5, 0.125, 1.0] and out[5, 21].tolist() == [1.0, 0.0, 0.5, 1.0]


# ---- partition ----------------------------------------------------------------------------------------------------------------------------------------------
def test_every_sample_inside_a_closed_mesh_is_covered_by_exactly_one_of_its_triangles(rendered8, P8):
    _, quad = rendered8["shared_edge_quad"]
    assert set(np.unique(quad["inside_count"])) == {0, 1}
    # the quad is 3.5 .. 30.5 x 2.5 .. 20.5: a sample is inside iff its coordinates are, the left and top edges included
    jj, ii = np.meshgrid(np.arange(24), np.arange(40), indexing="ij")
    x, y = 256 * ii[..., None] + P8[:, 0], 256 * jj[..., None] + P8[:, 1]
    np.testing.assert_array_equal(quad["inside_count"] == 1, (x >= 896) & (x < 7808) & (y >= 640) & (y < 5248))
    _, fan = rendered8["fan_around_a_pixel_centre"]
    assert set(np.unique(fan["inside_count"])) == {0, 1} and (fan["inside_count"][10, 18] == 1).all() and (fan["inside_count"][8:13, 14:23] == 1).all()
    for k in range(surface_cases.NUM_SOUPS):   # a soup is no mesh: what holds there is that no sample is lost or doubled between the two parts of a cut triangle
        s = surface_cases.random_soup(k)
        one = dict(s, draws=[dict(d, indices=d["indices"][:1], instance_ids=None if d["instance_ids"] is None else d["instance_ids"][:1], num_drawn=1) for d in s["draws"][:1]])
        assert mr.render(one, P8)["inside_count"].max() <= 1, k


def test_a_sliver_that_covers_samples_and_no_centre_exists_at_eight_samples_only(rendered8):
    s, r = rendered8["sliver_between_centres"]
    assert owned(r, 10, 20) == [0, 7] and int((r["store"] & LOW != 0).sum()) == 2 and r["stats"]["no_centre_primitives"] == 2
    assert not (mr.render(s, host.msaa_sample_positions(1))["store"] & LOW).any()
    assert not (surface_ref.render(s)["keys"] & LOW).any()


# ---- what the cases reach -----------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_were_built_to_reach(rendered8, P8):
    weights, owners, clipped2 = set(), 0, 0
    for name, (s, r) in rendered8.items():
        L8 = mr.layers(r["store"], 8)
        weights |= set(np.unique(L8["weights"]).tolist())
        owners = max(owners, int((L8["weights"] > 0).sum(0).max()))
        clipped2 += mr.layers(r["store"], 2)["clipped"]
        assert L8["clipped"] == 0, name
    _, cut = rendered8["cutout_at_the_edge"]
    _, near = rendered8["near_plane"]
    s = cases.CASES["staircase"]()
    halves = np.concatenate([mr.render(s, P8, rows=(0, 11))["store"], mr.render(s, P8, rows=(11, 24))["store"]])
    print(f"weights {sorted(weights)}, most owners a pixel {owners}, pixels clipped at two layers {clipped2}, cutout fragments with the centre outside: "
          f"{cut['stats']['centre_outside_kept']} kept, {cut['stats']['centre_outside_discarded']} discarded, edge pixels of cut parts {near['stats']['cut_on_edge_pixel']}")
    assert weights >= set(range(1, 9)) and owners == 8 and clipped2 > 0
    assert cut["stats"]["centre_outside_kept"] > 0 and cut["stats"]["centre_outside_discarded"] > 0
    # ... and the discard shows: column 20 of the kept rectangle holds its order at samples 3, 4, 5 (sx = 80, 48, 16), of the discarded one the opaque one's
    kept, gone = (cut["store"][5, 20] & LOW).astype(np.int64), (cut["store"][13, 20] & LOW).astype(np.int64)
    assert sorted(np.nonzero(kept > 4)[0].tolist()) == [3, 4, 5] and (gone <= 4).all() and (gone > 0).all()
    assert (np.asarray(cut["store"][13, 19] & LOW, np.int64) > 8).all()      # one column further in the same rectangle keeps
    assert near["stats"]["cut_parts"] >= 3 and near["stats"]["cut_on_edge_pixel"] > 0
    np.testing.assert_array_equal(halves, rendered8["staircase"][1]["store"])
    big = rendered8["triangle_larger_than_the_frame"][1]
    assert (big["store"] & LOW != 0).all()


# ---- layers and the accumulate ------------------------------------------------------------------------------------------------------------------------------
def test_weights_and_uncovered_sum_to_the_sample_count_and_clipping_folds_into_the_last_layer(rendered8):
    for name, (s, r) in rendered8.items():
        for L in (1, 2, 5, 8):
            got = mr.layers(r["store"], L)
            total = got["weights"].astype(np.int64).sum(0) + got["uncovered"]
            assert (total == 8).all(), (name, L)
            assert (got["counts"] == [(got["keys"][k] & LOW != 0).sum() for k in range(L)]).all()
            assert ((got["weights"] > 0) == (got["keys"] & LOW != 0)).all()
    _, r = rendered8["eight_owners"]
    full, two = mr.layers(r["store"], 8), mr.layers(r["store"], 2)
    assert (full["weights"][:, 5, 20] == 1).all() and two["weights"][:, 5, 20].tolist() == [1, 7] and two["clipped"] >= 7
    np.testing.assert_array_equal(two["keys"], full["keys"][:2])
    orders = (full["keys"][:, 5, 20] & LOW).astype(np.int64)
    assert (np.diff(orders) > 0).all()                                       # the layers come in primitive order
    for S in (2, 4):   # the other sample counts: the same sums
        st = mr.render(cases.CASES["staircase"](), host.msaa_sample_positions(S))["store"]
        got = mr.layers(st, S)
        assert (got["weights"].astype(np.int64).sum(0) + got["uncovered"] == S).all()


def test_a_fully_owned_pixel_takes_the_colours_bits_over_a_nan_and_an_infinity():
    weight = np.array([[8, 8, 4, 4, 0, 3]], np.uint8)
    uncovered = np.array([[0, 0, 4, 0, 8, 5]], np.uint8)
    target = np.zeros((1, 6, 4), f32)
    target[0, 0] = np.nan; target[0, 1] = np.inf; target[0, 2] = (1, 2, 3, 4); target[0, 3] = np.nan; target[0, 4] = (np.nan, np.inf, -np.inf, 5); target[0, 5] = np.inf
    colour = np.zeros((1, 6, 4), f32)
    colour[0, :] = (0.1, 0.7, 0.3, 1.0)
    colour[0, 1] = np.array([0x7FC01234, 0xFF800000, 0x00000001, 0x80000000], np.uint32).view(f32)   # a NaN payload, -inf, a denormal, -0: bits, not values
    out = mr.accumulate(target, colour, weight, uncovered, 8, 0)
    assert out.view(np.uint32)[0, 0].tolist() == colour.view(np.uint32)[0, 0].tolist() and out.view(np.uint32)[0, 1].tolist() == colour.view(np.uint32)[0, 1].tolist()
    half = f32(0.5)
    assert out[0, 2].tolist() == [half * f32(1) + half * f32(0.1), half * f32(2) + half * f32(0.7), half * f32(3) + half * f32(0.3), half * f32(4) + half * f32(1)]
    assert out[0, 3].tolist() == [half * f32(0.1), half * f32(0.7), half * f32(0.3), half]           # u = 0: the NaN under it is omitted, not multiplied by 0
    assert out.view(np.uint32)[0, 4].tolist() == target.view(np.uint32)[0, 4].tolist()                # w = 0: untouched
    assert np.isinf(out[0, 5]).all()                                                                  # a covered part over an infinity stays infinite
    later = mr.accumulate(out, colour, np.array([[0, 1, 4, 4, 0, 0]], np.uint8), uncovered, 8, 3)
    assert later.view(np.uint32)[0, 0].tolist() == out.view(np.uint32)[0, 0].tolist() and later[0, 3].tolist() == [f32(x) + f32(x) for x in out[0, 3]]
    z, avg = mr.depth_out(np.array([[[np.uint64(np.array(v, f32).view(np.uint32)) << np.uint64(32) | np.uint64(7) for v in (0.5, 0.25, 0.75, 1.0)]]], np.uint64))
    assert z.tolist() == [[[0.5, 0.25, 0.75, 1.0]]] and avg.tolist() == [[0.625]]


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------
def test_every_host_side_refusal_in_the_stand_alone_program(tmp_path):
    """scripts/msaa_host_check.cpp -- every refusal of the six entries, the store's size arithmetic and the packed sample table, against a context that never
    reaches a device -- built as a program of its own with the host sanitizers and run (a few seconds)"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "sailor_amd" / "csrc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc here")
    exe = tmp_path / "msaa_host_check"
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", f"-I{csrc}", str(ROOT / "scripts" / "msaa_host_check.cpp"), "-o", str(exe), f"-L{csrc}", "-lsailor_hip",
                            f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "msaa_host_check: ok" in run.stdout, run.stdout + run.stderr
