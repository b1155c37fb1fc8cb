"""The shade kernels' prologue and epilogue on the smallest frames at which their paths differ: quadrants that lie wholly inside the frame (the tile's origin
folded into a scalar base, one 32-bit byte offset per lane) beside quadrants that cross its right and bottom edge in the same launch, bands whose first
framebuffer row is not 0, lists of exactly 0 / 1 / 63 / 64 / 65 / 127 / 128 entries, a list that ends at an index that is no light's in every slot that
matters to the two staging waves, a roughness-0 pixel in one quadrant only, a directional light in either list half, and the kernels with 64-bit
pixel indices against the 32-bit ones.

The lists are WRITTEN by the test, not culled: the canonical lightsGrid / culledLights or the cull's per-tile slots, filled with the lengths and entries
the case is about.  The reference is the C oracle on the same lists with the tolerance and the helper of tests/test_shade_gpu.py; the four entry forms
(plain, _p, _t, _pt) of one case are equal bit for bit, as in tests/test_ambient_gpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from sailor_amd import host, synth
from sailor_amd.forward_plus import ForwardPlus, PreparedLights, upload_lights
from test_shade_gpu import assert_radiance_close

pytestmark = pytest.mark.gpu
FORMS = {"": (False, False), "_p": (False, True), "_t": (True, False), "_pt": (True, True)}   # suffix -> (the cull's tile lists, prepared lights)
SIZES = [(16, 16), (48, 32), (37, 21), (131, 77)]   # whole tiles only (one tile; 3 x 2), ragged right and bottom tiles beside whole ones (3 x 2; 9 x 5)
LENGTHS = (0, 1, 63, 64, 65, 127, 128)
NO_LIGHT = 0xFFFFFFFF
N_LIGHTS = 160
VARIANTS = [f"len{n}" for n in LENGTHS] + ["mixed", "end0", "end63", "end64", "end127", "rough0", "dir0", "dir64"]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(size, variant):
    """the frame, its lights, the lists (lens[t], entries[t, 128]) of every tile and the C oracle's radiance -- computed once per (size, variant)"""
    W, H = size
    c = Case()
    c.cam = synth.make_camera(W, H)
    c.depth = synth.make_linear_depth(W, H, 7, d_min=20.0, d_max=60.0)
    # (radii of the order of the scene's depth: most lights reach most pixels, so that a slot read wrongly shows in the picture)
    c.lights = synth.make_lights(c.cam, c.depth, synth.LightSetConfig(count=N_LIGHTS, radius_scale=60.0, spot_fraction=0.4, d_min=15.0, d_max=70.0), 7)
    c.surface = synth.make_surface(c.cam, c.depth, 7)
    Tx, Ty = host.num_tiles(W, H)
    T = Tx * Ty
    rng = np.random.default_rng(1000 * W + H)
    c.entries = np.stack([rng.permutation(N_LIGHTS)[:128] for _ in range(T)]).astype(np.uint32)
    c.lens = np.full(T, 128, np.uint32)
    if variant.startswith("len"):        # every list of exactly this length
        c.lens[:] = int(variant[3:])
    elif variant == "mixed":             # every length in one launch (as many of them as the frame has tiles), neighbours differ
        c.lens = np.array([(65, 0, 128, 1, 64, 127, 63)[(t + t // Tx) % len(LENGTHS)] for t in range(T)], np.uint32)
    elif variant.startswith("end"):      # the list ends at this slot in all four waves
        c.entries[:, int(variant[3:])] = NO_LIGHT
    elif variant == "rough0":            # one pixel of quadrant 2 (upper left) of tile 0: that wave alone leaves the usual path
        c.surface[1, H - 1 - 11, 3, 3] = 0.0
        c.lens[:] = 70
    else:                                # a directional light in slot 0 / slot 64 of every list, and nowhere else
        slot = int(variant[3:])
        c.lights["type"][5] = host.LIGHT_DIRECTIONAL
        for t in range(T):
            others = c.entries[t][c.entries[t] != 5]
            c.entries[t, :127] = others[:127]
            c.entries[t, 127] = c.entries[t, slot]
            c.entries[t, slot] = 5
    c.grid = np.zeros((T, 2), np.uint32)
    c.grid[:, 0] = 1 + 128 * np.arange(T)
    c.grid[:, 1] = c.lens
    c.indices = np.zeros(1 + 128 * T, np.uint32)
    c.indices[0] = c.lens.sum()
    c.indices[1:] = c.entries.ravel()
    c.ref = oracle.shade(c.cam.frame, W, H, c.surface, c.lights, c.grid, c.indices, None)
    return c


def as_bytes(a, device):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).ravel().copy()).to(device)


def gpu_shade(ctx, c, form, band=None, band_form=False):
    """one band of the case through one entry form, from lists written here -> (radiance, launched kernel names, framebuffer rows).
    band_form: the band's list lengths as bytes where the cull leaves them, so that a partial band takes the band kernels (long tiles go to the split blocks)"""
    W, H = c.cam.width, c.cam.height
    tile_lists, prep = FORMS[form]
    dev = ctx.device
    l = upload_lights(c.lights, dev)
    fp = ForwardPlus(ctx, W, H, N_LIGHTS, band=band, prepared=PreparedLights(ctx, l, N_LIGHTS) if prep else None)
    b = fp.band
    rows = slice(b.fbRowBegin, b.fbRowBegin + b.fbRowCount)
    t0, nt = b.tileRowBegin * fp.Tx, fp.band_tiles
    lens, entries = c.lens[t0:t0 + nt], c.entries[t0:t0 + nt]
    ws, base = fp.workspace, fp.workspace.data_ptr()
    if tile_lists:
        ws[fp.tile_num - base: fp.tile_num - base + 4 * nt] = as_bytes(lens, dev)
        ws[fp.tile_lists - base: fp.tile_lists - base + 512 * nt] = as_bytes(entries, dev)
    else:
        grid = np.stack([1 + 128 * np.arange(nt), lens], 1).astype(np.uint32)
        fp.grid = torch.from_numpy(grid.view(np.int32).ravel().copy()).to(dev)
        fp.culled = torch.from_numpy(np.concatenate([[lens.sum()], entries.ravel()]).astype(np.uint32).view(np.int32)).to(dev)
    if band_form:
        ws[fp.tile_order - base: fp.tile_order - base + nt] = as_bytes(lens.astype(np.uint8), dev)
    fp.shade_from_tile_lists = tile_lists
    fp.use_tile_order = band_form
    fp._culled_once = tile_lists or band_form   # (the lists are there: written above)
    s = torch.from_numpy(np.ascontiguousarray(c.surface[:, rows])).to(dev)
    out = []
    names = ctx.launches_of(lambda: out.append(fp.shade(c.cam.frame, s, l, N_LIGHTS, None)))
    ctx.synchronize()
    return out[0].cpu().numpy(), names, rows


def assert_forms_agree(ctx, c, kernel, band=None, band_form=False):
    first = None
    for form in FORMS:
        got, names, rows = gpu_shade(ctx, c, form, band, band_form)
        assert names == [kernel + form], (form, names)
        assert_radiance_close(got, c.ref[rows])
        if first is None:
            first = got
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), f"form '{form}' differs from form '' in {(got != first).sum()} values"
    return first


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("size", SIZES)
def test_whole_frame(ctx, size, variant):
    c = make_case(size, variant)
    lit = c.ref[..., :3].sum(-1) > 0
    if variant in ("end0", "len0"):
        assert not lit.any(), "an empty list, or one that ends at slot 0, lights nothing"
    elif variant == "len1":
        assert lit.any()
    elif variant != "mixed":
        assert lit.mean() > 0.5, "the lights must reach the surface, or a wrong list would not show"
    assert_forms_agree(ctx, c, "k2_shade")


def test_the_variants_are_different_pictures():
    """(CPU part of the above: what a case is about changes the oracle's picture -- a kernel that ignored it would not pass)"""
    size = (48, 32)
    full = make_case(size, "len128").ref
    for variant in ("end63", "end64", "end127", "mixed", "dir0", "len1", "len63", "len64", "len65", "len127"):
        assert np.abs(make_case(size, variant).ref[..., :3] - full[..., :3]).max() > 1e-3, variant
    a, b = make_case(size, "end63").ref, make_case(size, "end64").ref
    assert np.abs(a[..., :3] - b[..., :3]).max() > 1e-4, "slot 63 is a light of its own"


@pytest.mark.parametrize("size, tile_rows", [((48, 32), (0, 1)), ((48, 32), (1, 2)), ((131, 77), (0, 3)), ((131, 77), (3, 5)), ((37, 21), (1, 2))])
@pytest.mark.parametrize("variant", ["mixed", "len65", "end64", "dir64"])
def test_bands(ctx, size, tile_rows, variant):
    """Bands cut at tile rows: (0, n) has its first framebuffer row above 0 -- whole at 48 x 32, ragged on the right at 131 x 77 -- and the last one
    holds the frame's ragged bottom row.  On the per-tile grid (no length bytes) and, with them, through the band kernels, whose long tiles go to the
    split blocks: four waves per quadrant, each with every fourth slot."""
    c = make_case(size, variant)
    W, H = size
    band = host.band_from_tile_rows(W, H, *tile_rows)
    assert (band.fbRowBegin != 0) == (tile_rows[1] * 16 < H)
    assert_forms_agree(ctx, c, "k2_shade", band)
    assert_forms_agree(ctx, c, "k2_shade_band", band, band_form=True)


@pytest.mark.parametrize("size", [(48, 32), (131, 77)])
def test_wide_addressing_equals_32_bit_addressing(ctx, size):
    """The kernels with 64-bit pixel indices (planes of 4 GB and more; forced here by SAILOR_SHADE_WIDE_ADDRESSING=1) against the 32-bit ones on the
    same small frame, whole and as a band with the band kernels: bit for bit."""
    c = make_case(size, "mixed")
    W, H = size
    band = host.band_from_tile_rows(W, H, 0, 1)
    for kernel, b, band_form in (("k2_shade", None, False), ("k2_shade", band, False), ("k2_shade_band", band, True)):
        narrow, names, rows = gpu_shade(ctx, c, "_pt", b, band_form)
        assert names == [kernel + "_pt"], names
        os.environ["SAILOR_SHADE_WIDE_ADDRESSING"] = "1"
        try:
            wide, names, _rows = gpu_shade(ctx, c, "_pt", b, band_form)
        finally:
            del os.environ["SAILOR_SHADE_WIDE_ADDRESSING"]
        assert names == [kernel + "_pt_w"], names
        assert_radiance_close(wide, c.ref[rows])
        assert np.array_equal(wide.view(np.uint32), narrow.view(np.uint32)), f"{kernel} {b}: {(wide != narrow).sum()} values differ"
