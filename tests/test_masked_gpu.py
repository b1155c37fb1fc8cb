"""The Masked queue (sailor_amd/csrc/surface_masked.hip) through the C-ABI against tests/masked_ref.py: keys, depth and coverage bit for bit, the three planes
bit for bit with non-finite values compared by class -- every case and every soup of tests/masked_cases.py with and without a prepass, with back-face culling,
in bands; the masked depth prepass; the draw without the flag through both entry points; the golden file; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import masked_cases as cases
import masked_ref
import surface_cases
import surface_ref as ref
from make_masked_golden import PATH as GOLDEN, masked_golden_scene
from sailor_amd import _lib, host
from sailor_amd.forward_plus import SurfacePass, masked_depth_prepass
from test_surface_gpu import assert_same, dev, frame_of

pytestmark = pytest.mark.gpu


def upload_textures(ctx, images, srgb):
    """forward_plus.upload_textures, with a descriptor without texels (NULL, 0 x 0) for an image of shape (0, 0, 4)"""
    keep, table = [], (_lib.TextureDesc * len(images))()
    for k, (img, s) in enumerate(zip(images, srgb)):
        img = np.ascontiguousarray(img, np.uint8)
        if img.shape[0] == 0 or img.shape[1] == 0:
            table[k] = _lib.TextureDesc(None, 0, 0, 0, 0)
            continue
        t = torch.from_numpy(img.view(np.uint32).reshape(img.shape[0], img.shape[1]).view(np.int32)).to(ctx.device)
        keep.append(t)
        table[k] = _lib.TextureDesc(t.data_ptr(), img.shape[1], img.shape[0], _lib.TEXTURE_SRGB if s else 0, 0)
    d = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(ctx.device)
    return d, len(images), keep + [d]


class Uploaded:
    """a scene's buffers on the device"""

    def __init__(self, ctx, s):
        self.s, self.frame = s, frame_of(s)
        self.instances = dev(ctx, s["instances"].view(np.uint8))
        self.materials = dev(ctx, s["materials"].view(np.uint8))
        self.textures, self.num_textures, self.keep = upload_textures(ctx, s["textures"], s["srgb"])
        self.draws = [dict(vertices=dev(ctx, d["vertices"]), indices=dev(ctx, d["indices"], np.int32), instance_ids=None if d["instance_ids"] is None else
                           dev(ctx, d["instance_ids"], np.int32), num_drawn=d["num_drawn"], first_instance=d["first_instance"], cull_back=d["cull_back"]) for d in s["draws"]]
        self.cutout = [bool(d.get("alpha_cutout", False)) for d in s["draws"]]

    def draw_all(self, sp, everything_through_the_masked_entry=False, cull_back=False):
        lib, ctx = sp.ctx._lib, sp.ctx
        for d, cut in zip(self.draws, self.cutout):
            d = dict(d, cull_back=d["cull_back"] or cull_back)
            if cut:
                sp.draw(self.frame, instances=self.instances, alpha_cutout=True, materials=self.materials, textures=self.textures, num_textures=self.num_textures, **d)
            elif not everything_through_the_masked_entry:
                sp.draw(self.frame, instances=self.instances, **d)
            else:   # a draw WITHOUT the flag through sailor_hip_surface_draw_masked (SurfacePass.draw routes by the flag, so by hand), no tables
                nt = d["indices"].numel() // 3
                nd = d["num_drawn"] if d["num_drawn"] is not None else (d["instance_ids"].numel() if d["instance_ids"] is not None else
                                                                       self.instances.numel() // 96 - d["first_instance"])
                desc = _lib.SurfaceDraw(d["vertices"].data_ptr(), d["indices"].data_ptr(), None if d["instance_ids"] is None else d["instance_ids"].data_ptr(), nt, nd,
                                        sp.prim_base, _lib.SURFACE_CULL_BACK if d["cull_back"] else 0, d["first_instance"], 0)
                _lib.check(lib.sailor_hip_surface_draw_masked(ctx.handle, C.byref(self.frame), C.byref(desc), self.instances.data_ptr(), None, 0, None, 0, sp.draw_index,
                                                              sp.W, sp.H, C.byref(sp.band), sp.workspace.data_ptr(), sp.workspace.numel()), "draw_masked", ctx.handle)
                sp.prim_base += host.surface_draw_prims(nt, nd)
                sp.draw_index += 1


def run(ctx, s, prepass=None, band=None, up=None, **how):
    """the scene through begin / draw or draw_masked / resolve -> dict like masked_ref.render's"""
    up = up or Uploaded(ctx, s)
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=max(len(s["draws"]), 1))
    sp.begin(None if prepass is None else dev(ctx, prepass), prim_base=s.get("prim_base", 0))
    up.draw_all(sp, **how)
    surface, depth, cov = sp.resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures)
    keys = sp.download_keys()
    return dict(planes=surface.cpu().numpy(), depth=depth.cpu().numpy(), covered=cov.cpu().numpy().astype(bool), keys=keys, sp=sp, up=up)


SCENES = list(cases.CASES) + [f"masked_soup_{seed}" for seed in range(cases.NUM_SOUPS)]


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: masked_ref.render(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


@pytest.mark.parametrize("name", SCENES)
def test_every_case_and_soup_against_the_restatement_with_and_without_a_prepass(ctx, scenes, rendered, name):
    s = scenes[name]
    up = Uploaded(ctx, s)
    got = run(ctx, s, up=up)
    assert_same(got, rendered[name], name)
    # pinned rule 1: at every pixel a cutout draw owns, P0.w is the alpha the draw tested -- so it survives the test
    a = got["planes"][0][..., 3][rendered[name]["cutout"]]
    assert ((a >= np.float32(0.5)) | np.isnan(a)).all(), name
    for what, pre in (("the opaque prepass", cases.opaque_prepass(s)), ("the opaque and the masked prepass", cases.full_prepass(s))):
        assert_same(run(ctx, s, prepass=pre, up=up), masked_ref.render(s, prepass=pre), f"{name} behind {what}")


def test_with_back_face_culling(ctx, scenes):
    for name in cases.CULL_BACK_CASES:
        c = surface_cases.with_cull_back(scenes[name])
        assert_same(run(ctx, c), masked_ref.render(c), f"{name} with back-face culling")


def test_two_bands_concatenate_to_the_whole_frame(ctx, scenes, rendered):
    for name in cases.BAND_CASES:
        s, whole = scenes[name], rendered[name]
        up, parts = Uploaded(ctx, s), []
        for rank in reversed(range(2)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
            band = host.band_for_rank(s["W"], s["H"], rank, 2)
            got = run(ctx, s, band=band, up=up)
            assert_same(got, masked_ref.render(s, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)), f"{name} band {rank}/2")
            parts.append(got)
        np.testing.assert_array_equal(np.concatenate([p["keys"] for p in parts]), whole["keys"])
        assert ref.same_bits_or_class(np.concatenate([p["planes"] for p in parts], axis=1), whole["planes"]).all()


def test_masked_depth_prepass(ctx, scenes):
    """begin(opaque depth), the masked draws, store_depth: the restatement's depth, the opaque depth bit for bit in every hole, and a RenderScene pass begun from
    it covers the same pixels"""
    for name in ("checker_over_opaque", "per_instance_materials", "large_checker_two_superblocks", "masked_soup_1", "masked_soup_12"):
        s = scenes[name]
        up = Uploaded(ctx, s)
        opaque = cases.opaque_prepass(s)
        depth = dev(ctx, opaque)
        sp = SurfacePass(ctx, s["W"], s["H"], max_draws=len(s["draws"]))
        out = masked_depth_prepass(sp, up.frame, depth, [d for d, cut in zip(up.draws, up.cutout) if cut], up.instances, up.materials, up.textures, up.num_textures)
        ctx.synchronize()
        assert out is depth
        got, want = depth.cpu().numpy(), cases.full_prepass(s)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=name)
        cut = dict(s, draws=[d for d in s["draws"] if d.get("alpha_cutout", False)])
        owned = masked_ref.render(cut, prepass=opaque)["covered"]
        assert owned.any() and (~owned).any(), name
        np.testing.assert_array_equal(got[~owned].view(np.uint32), opaque[~owned].view(np.uint32), err_msg=f"{name}: the holes")
        scene_pass, no_prepass = run(ctx, s, prepass=got, up=up), masked_ref.render(s)
        assert_same(scene_pass, masked_ref.render(s, prepass=want), f"{name}: RenderScene from the masked prepass")
        if name == "checker_over_opaque":   # (the soups draw cutout geometry in the first draw too: only here is the prepass the scene's own depth)
            np.testing.assert_array_equal(scene_pass["covered"], no_prepass["covered"])
    # in two bands into one whole-frame attachment
    s = scenes["large_checker_two_superblocks"]
    up, depth = Uploaded(ctx, s), torch.zeros((s["H"], s["W"]), dtype=torch.float32, device=ctx.device)
    for rank in range(2):
        sp = SurfacePass(ctx, s["W"], s["H"], host.band_for_rank(s["W"], s["H"], rank, 2), max_draws=1)
        sp.begin(depth)
        up.draw_all(sp)
        sp.store_depth(depth)
    ctx.synchronize()
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), cases.full_prepass(s).view(np.uint32))


def test_a_draw_without_the_flag_writes_the_same_keys_through_both_entry_points(ctx, scenes):
    for name, s in [("flag_absent", scenes["flag_absent"]), ("near_plane", surface_cases.near_plane()), ("larger", surface_cases.triangle_larger_than_the_frame()),
                    ("soup", surface_cases.random_soup(3))]:
        up = Uploaded(ctx, s)
        plain, masked = run(ctx, s, up=up), run(ctx, s, up=up, everything_through_the_masked_entry=True)
        np.testing.assert_array_equal(plain["keys"], masked["keys"], err_msg=name)
        assert_same(masked, ref.render(s), name)
        launched = ctx.launches_of(lambda: (masked["sp"].begin(), up.draw_all(masked["sp"], everything_through_the_masked_entry=True)))
        assert set(launched[1:]) == {"k_surface_visibility_masked"}, launched
        ctx.synchronize()


def test_golden_through_the_c_abi(ctx):
    g = np.load(GOLDEN)
    got = run(ctx, masked_golden_scene(g))   # inputs from the file alone
    np.testing.assert_array_equal(got["keys"], g[f"{cases.GOLDEN_CASE}.keys"])
    assert ref.same_bits_or_class(got["planes"], g[f"{cases.GOLDEN_CASE}.planes"]).all()


def test_refusals_launch_nothing_and_say_why(ctx, scenes):
    lib = ctx._lib
    s = scenes["checker_over_opaque"]
    W, H = s["W"], s["H"]
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, W, H, max_draws=2)
    sp.begin()
    ws, n = sp.workspace.data_ptr(), sp.workspace.numel()
    band, frame = sp.band, up.frame
    d = up.draws[1]
    bad_band = _lib.Band(0, 1, 3, 16)
    depth = torch.zeros(H * W + 1, dtype=torch.float32, device=ctx.device)
    CUT = _lib.SURFACE_ALPHA_CUTOUT

    def desc(flags=CUT, vertices=d["vertices"].data_ptr(), prim_base=0):
        return _lib.SurfaceDraw(vertices, d["indices"].data_ptr(), d["instance_ids"].data_ptr(), 2, 1, prim_base, flags, 0, 0)

    def draw_call(dd, index=0, workspace=ws, size=n, b=band, inst=up.instances.data_ptr(), mats=up.materials.data_ptr(), nm=2, tex=up.textures.data_ptr(), ntex=up.num_textures):
        return lambda: lib.sailor_hip_surface_draw_masked(ctx.handle, C.byref(frame), C.byref(dd), inst, mats, nm, tex, ntex, index, W, H, C.byref(b), workspace, size)

    def store_call(workspace=ws, size=n, out=depth.data_ptr(), b=band):
        return lambda: lib.sailor_hip_surface_store_depth(ctx.handle, workspace, size, out, W, H, C.byref(b))
    misuse = {
        "draw_masked: the flag with null materials": draw_call(desc(), mats=None),
        "draw_masked: the flag with null textures": draw_call(desc(), tex=None),
        "draw_masked: the flag with no materials": draw_call(desc(), nm=0),
        "draw_masked: the flag with no textures": draw_call(desc(), ntex=0),
        "draw_masked: unknown flag bits": draw_call(desc(flags=CUT | 4)),
        "draw_masked: unknown flag bits alone": draw_call(desc(flags=0x80000000)),
        "draw_masked: null vertices": draw_call(desc(vertices=None)),
        "draw_masked: null instances": draw_call(desc(), inst=None),
        "draw_masked: null workspace": draw_call(desc(), workspace=None),
        "draw_masked: workspace too small": draw_call(desc(), size=1000),
        "draw_masked: drawIndex >= maxDraws": draw_call(desc(), index=2),
        "draw_masked: primBase overflow": draw_call(desc(prim_base=2 ** 32 - 1 - 4)),
        "draw_masked: invalid band": draw_call(desc(), b=bad_band),
        "draw: the flag through the plain entry point": lambda: lib.sailor_hip_surface_draw(ctx.handle, C.byref(frame), C.byref(desc()), up.instances.data_ptr(), 0, W, H,
                                                                                           C.byref(band), ws, n),
        "store_depth: workspace too small": store_call(size=lib.sailor_hip_surface_keys_offset() + W * H * 8),
        "store_depth: null workspace": store_call(workspace=None),
        "store_depth: misaligned depth": store_call(out=depth.data_ptr() + 2),
        "store_depth: null depth": store_call(out=None),
        "store_depth: invalid band": store_call(b=bad_band),
    }
    for what, call in misuse.items():
        before, _ = ctx.launch_log(0)
        assert call() == -1, what
        after, _ = ctx.launch_log(0)
        assert after == before, f"{what}: launched {after - before} kernels"
        assert b"sailor_hip_surface_" in lib.sailor_hip_context_last_error(ctx.handle), what
    assert b"ALPHA_CUTOUT needs materials and textures" in (draw_call(desc(), mats=None)(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"unknown flags" in (draw_call(desc(flags=CUT | 4))(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"depth attachment" in (store_call(out=depth.data_ptr() + 2)(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    # without the flag the tables may be absent; the largest primBase still accepted
    assert draw_call(desc(flags=0), mats=None, nm=0, tex=None, ntex=0)() == 0
    assert draw_call(desc(prim_base=2 ** 32 - 2 - 4), index=1)() == 0
    ctx.synchronize()
    names = ctx.launches_of(lambda: (sp.begin(), up.draw_all(sp), sp.store_depth(depth[:H * W].view(H, W))))
    assert names == ["k_surface_begin", "k_surface_visibility", "k_surface_visibility_masked", "k_surface_store_depth"], names
    ctx.synchronize()
