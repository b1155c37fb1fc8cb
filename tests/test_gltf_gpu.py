"""glTF materials (sailor_amd/csrc/surface_gltf.hip) through the C-ABI against tests/gltf_ref.py: keys, depth and coverage bit for bit; the three planes, the
emissive plane and aoOut bit for bit with non-finite words compared by class -- every case and every soup of tests/gltf_cases.py with and without a prepass, with
back-face culling, in bands; the Standard scenes through sailor_hip_surface_resolve_gltf against sailor_hip_surface_resolve; the composite; one frame through
the shade against the float64 oracle; the golden file; the refusals; the launch times at 3840 x 2160."""
import ctypes as C

import numpy as np
import pytest
import torch

import gltf_cases as cases
import gltf_ref
import masked_cases
import surface_cases
import surface_ref as ref
from make_gltf_golden import OUTPUTS, PATH as GOLDEN
from oracle import oracle, oracle_f64
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import ForwardPlus, SurfacePass, linearize_depth, upload_ibl, upload_lights
from test_masked_gpu import upload_textures
from test_surface_gpu import dev, frame_of

pytestmark = pytest.mark.gpu


class Uploaded:
    """a scene's buffers on the device"""

    def __init__(self, ctx, s):
        self.s, self.frame = s, frame_of(s)
        self.instances = dev(ctx, s["instances"].view(np.uint8))
        self.materials = dev(ctx, s["materials"].view(np.uint8))
        self.textures, self.num_textures, self.keep = upload_textures(ctx, s["textures"], s["srgb"])
        spare = torch.zeros(3, dtype=torch.int32, device=ctx.device)
        self.draws = [dict(vertices=dev(ctx, d["vertices"]), indices=dev(ctx, d["indices"], np.int32) if len(d["indices"]) else spare[:0], instance_ids=None
                           if d["instance_ids"] is None else dev(ctx, d["instance_ids"], np.int32), num_drawn=d["num_drawn"], first_instance=d["first_instance"],
                           cull_back=d["cull_back"], alpha_cutout=bool(d.get("alpha_cutout", False)), gltf=bool(d.get("gltf", False))) for d in s["draws"]]
        self.ao_in = None if s.get("ao_in") is None else np.asarray(s["ao_in"], np.float32)

    def draw_all(self, sp, cull_back=False):
        for d in self.draws:
            d = dict(d, cull_back=d["cull_back"] or cull_back)
            tables = dict(materials=self.materials, textures=self.textures, num_textures=self.num_textures) if d["alpha_cutout"] or d["gltf"] else {}
            sp.draw(self.frame, instances=self.instances, **tables, **d)


def run(ctx, s, prepass=None, band=None, up=None, ao_in="scene", **how):
    """the scene through begin / the three draw entry points / resolve_gltf -> dict like gltf_ref.render's"""
    up = up or Uploaded(ctx, s)
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=max(len(s["draws"]), 1))
    sp.begin(None if prepass is None else dev(ctx, prepass), prim_base=s.get("prim_base", 0))
    up.draw_all(sp, **how)
    ao = up.ao_in if isinstance(ao_in, str) else ao_in
    rows = slice(sp.band.fbRowBegin, sp.band.fbRowBegin + sp.band.fbRowCount)
    d_ao = None if ao is None else dev(ctx, ao[rows])
    surface, depth, cov, ao_out, emissive = sp.resolve_gltf(up.frame, up.instances, up.materials, up.textures, up.num_textures, ao_in=d_ao)
    keys = sp.download_keys()
    return dict(planes=surface.cpu().numpy(), depth=depth.cpu().numpy(), covered=cov.cpu().numpy().astype(bool), keys=keys, ao_out=ao_out.cpu().numpy(),
                emissive=emissive.cpu().numpy(), sp=sp, up=up, surface=surface, d_emissive=emissive, d_ao_out=ao_out)


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got["keys"], want["keys"], err_msg=f"{what}: keys")
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), err_msg=f"{what}: depth")
    np.testing.assert_array_equal(got["covered"], want["covered"], err_msg=f"{what}: coverage")
    for k in ("planes", "emissive", "ao_out"):
        same = ref.same_bits_or_class(got[k], want[k])
        assert same.all(), f"{what}: {(~same).sum()} words of {k} differ, first at {np.argwhere(~same)[:4].tolist()}"


SCENES = list(cases.CASES) + [f"gltf_soup_{seed}" for seed in range(cases.NUM_SOUPS)]


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: gltf_ref.render(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


@pytest.mark.parametrize("name", SCENES)
def test_every_case_and_soup_against_the_restatement_with_and_without_a_prepass(ctx, scenes, rendered, name):
    s = scenes[name]
    up = Uploaded(ctx, s)
    assert_same(run(ctx, s, up=up), rendered[name], name)
    for what, pre in (("the opaque prepass", cases.opaque_prepass(s)), ("the opaque and the masked prepass", cases.full_prepass(s))):
        assert_same(run(ctx, s, prepass=pre, up=up), gltf_ref.render(s, prepass=pre), f"{name} behind {what}")


def test_with_back_face_culling(ctx, scenes):
    kept = []
    for name in cases.CULL_BACK_CASES:
        c = surface_cases.with_cull_back(scenes[name])
        want = gltf_ref.render(c)
        kept.append(int(want["covered"].sum()))
        assert_same(run(ctx, c), want, f"{name} with back-face culling")
    assert sum(k > 50 for k in kept) >= 2 and 0 in kept, kept   # front faces survive, a wholly back-facing scene leaves nothing


STANDARD_SCENES = [("surface", name) for name in surface_cases.CASES] + [("masked", name) for name in masked_cases.CASES] + \
                  [("masked", f"masked_soup_{seed}") for seed in range(masked_cases.NUM_SOUPS)]


@pytest.fixture(scope="module")
def standard_scenes():
    out = {("surface", name): build() for name, (build, _) in surface_cases.CASES.items()}
    out.update({("masked", name): s for name, s in masked_cases.all_scenes().items()})
    return out


@pytest.mark.parametrize("which", STANDARD_SCENES, ids=lambda w: f"{w[0]}-{w[1]}")
def test_standard_scenes_resolve_as_sailor_hip_surface_resolve_does(ctx, standard_scenes, which):
    """drawn with the existing draw entry points, resolve_gltf writes sailor_hip_surface_resolve's planes, depth and coverage bit for bit, emissive (0, 0, 0, 1)
    and aoOut = aoIn's bits (a NaN among them), with and without an aoIn"""
    s = standard_scenes[which]
    rng = np.random.default_rng(len(which[1]))
    ao = rng.uniform(0, 2, (s["H"], s["W"])).astype(np.float32)
    ao[0, 0], ao[s["H"] // 2, s["W"] // 2] = np.nan, np.inf
    got = run(ctx, s, ao_in=ao)
    sp, up = got["sp"], got["up"]
    surface, depth, cov = sp.resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures)
    for a, b in ((got["surface"], surface), (torch.from_numpy(got["depth"]), depth.cpu()), (torch.from_numpy(got["ao_out"]), torch.from_numpy(ao))):
        np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32), err_msg=str(which))
    np.testing.assert_array_equal(got["covered"], cov.cpu().numpy().astype(bool))
    assert (got["emissive"] == gltf_ref.NO_EMISSIVE).all()
    assert (run(ctx, s, ao_in=None, up=up)["ao_out"] == 1).all()


def test_an_opaque_gltf_draw_issues_the_keys_of_sailor_hip_surface_draw(ctx):
    for name in ("near_plane", "multiple_draws", "instance_indirection", "triangle_larger_than_the_frame", "degenerates", "multiple_draws_high_prim_base"):
        s = surface_cases.CASES[name][0]()
        plain, as_gltf = run(ctx, s), run(ctx, cases.as_gltf(s))
        np.testing.assert_array_equal(plain["keys"], as_gltf["keys"], err_msg=name)
        launched = ctx.launches_of(lambda: (as_gltf["sp"].begin(), as_gltf["up"].draw_all(as_gltf["sp"])))
        assert set(launched[1:]) == {"k_surface_visibility_gltf"}, launched
        ctx.synchronize()


def test_two_bands_concatenate_to_the_whole_frame(ctx, scenes, rendered):
    for name in cases.BAND_CASES:
        s, whole = scenes[name], rendered[name]
        up, parts = Uploaded(ctx, s), []
        for rank in reversed(range(2)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
            band = host.band_for_rank(s["W"], s["H"], rank, 2)
            got = run(ctx, s, band=band, up=up)
            assert_same(got, gltf_ref.render(s, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)), f"{name} band {rank}/2")
            parts.append(got)
        np.testing.assert_array_equal(np.concatenate([p["keys"] for p in parts]), whole["keys"])
        for k, axis in (("planes", 1), ("emissive", 0), ("ao_out", 0)):
            assert ref.same_bits_or_class(np.concatenate([p[k] for p in parts], axis=axis), whole[k]).all(), (name, k)


def test_composite_adds_the_emissive_term_behind_the_radiance(ctx, scenes, rendered):
    """covered: emissive.rgb + radiance.rgb with one fp32 add per channel, radiance's alpha; uncovered: the target's bits -- non-finite values among all three"""
    for name in ("mixed_pass", "emissive_srgb"):
        s, want = scenes[name], rendered[name]
        got = run(ctx, s)
        rng = np.random.default_rng(4)
        rad, tgt = (rng.uniform(-2, 4, (s["H"], s["W"], 4)).astype(np.float32) for _ in range(2))
        rad[1, 2], rad[3, 4, 1], tgt[5, 6] = np.nan, np.inf, np.nan
        out = got["sp"].composite_gltf(dev(ctx, rad), got["d_emissive"], dev(ctx, tgt)).cpu().numpy()
        expect = gltf_ref.composite(rad, want["emissive"], want["covered"], tgt)
        c = want["covered"]
        assert c.any() and (~c).any() and (want["emissive"][c][:, :3] > 0).any()
        assert ref.same_bits_or_class(out[c], expect[c]).all(), name
        np.testing.assert_array_equal(out[~c].view(np.uint32), tgt[~c].view(np.uint32))
        np.testing.assert_array_equal(out[c][:, 3].view(np.uint32), rad[c][:, 3].view(np.uint32))


def test_golden_through_the_c_abi(ctx):
    g = np.load(GOLDEN)
    for name in cases.GOLDEN_CASES:
        got = run(ctx, cases.scene_from_arrays(g, name))   # inputs from the file alone
        np.testing.assert_array_equal(got["keys"], g[f"{name}.keys"])
        for k in OUTPUTS[1:]:
            assert ref.same_bits_or_class(got[k], g[f"{name}.{k}"]).all(), (name, k)


# ---- one frame through the shade ------------------------------------------------------------------------------------------------------------------------
def end_to_end_scene(W=48, H=32):
    """glTF boxes (two materials: one emissive with an orm and an occlusion texture, one cutout) on a glTF ground under the synthetic camera, six point lights
    among them and an IBL set whose ao is not constant"""
    cam = synth.make_camera(W, H)
    fb = np.frombuffer(bytes(cam.frame), np.float32)
    rng = np.random.default_rng(17)
    box = surface_cases.boxes_and_ground(1, W, H)["draws"][0]
    num = 7
    models = [host.transform_matrix([rng.uniform(-45, 45), rng.uniform(128, 150), rng.uniform(-110, -35), 1.0], (lambda q: q / np.linalg.norm(q))(rng.normal(size=4)),
                                    [*rng.uniform(5, 14, 3), 1.0]) for _ in range(num)] + [surface_cases.IDENTITY]
    g = [surface_cases.vertex((-300, 120, -5), (0, 0), normal=(0, 1, 0), tangent=(1, 0, 0), bitangent=(0, 0, -1)),
         surface_cases.vertex((300, 120, -5), (9, 0), normal=(0, 1, 0), tangent=(1, 0, 0), bitangent=(0, 0, -1)),
         surface_cases.vertex((300, 120, -400), (9, 9), normal=(0, 1, 0), tangent=(1, 0, 0), bitangent=(0, 0, -1)),
         surface_cases.vertex((-300, 120, -400), (0, 9), normal=(0, 1, 0), tangent=(1, 0, 0), bitangent=(0, 0, -1))]
    orm, occ = cases.rgb_texture(4, 4, 3), cases.rgb_texture(4, 4, 31)
    orm[..., 1] = np.random.default_rng(6).integers(150, 256, (4, 4))   # roughness away from 0, where NdfGGX is ill-conditioned in fp32
    occ[..., 0] = np.random.default_rng(5).integers(200, 256, (4, 4))   # sRGB 200..255 decodes to 0.58..1: on both sides of the set's ao
    mats = [cases.gltf_material(base=(0.9, 0.8, 0.7, 1), emissive=(0.6, 0.3, 0.1, 0), metallic=0.7, roughness=0.8, normal_scale=0.7, samplers=(0, 1, 2, 3, 2)),
            cases.gltf_material(base=(0.4, 0.6, 0.9, 1), emissive=(0.0, 0.2, 0.4, 0), metallic=0.3, roughness=0.9, cutoff=0.4, samplers=(4, 1, 2, 3, 0)),
            cases.gltf_material(base=(0.5, 0.7, 0.4, 1), metallic=0.2, roughness=0.6, samplers=(0, 1, 2, 3, 0))]
    s = surface_cases.scene(W, H, fb[16:32].copy(), [cases.gltf(surface_cases.draw(box["vertices"], box["indices"], first_instance=0, num_drawn=4, cull_back=True)),
                                                     cases.cutout(cases.gltf(surface_cases.draw(box["vertices"], box["indices"], first_instance=4, num_drawn=num - 4))),
                                                     cases.gltf(surface_cases.draw(g, [(0, 1, 2), (0, 2, 3)], first_instance=num, num_drawn=1))],
                            models=models, view=fb[0:16].copy(),
                            textures=[surface_cases.distinct_texture(8, 8, 2), cases.tilted_normal_map(), orm, occ, masked_cases.checker(4)],
                            srgb=[True, False, True, True, True], mats=mats, inst_materials=[0, 0, 0, 0, 1, 1, 1, 2])
    lights = np.zeros(6, host.LIGHT_DTYPE)
    lights["worldPosition"] = np.stack([rng.uniform(-50, 50, 6), rng.uniform(135, 160, 6), rng.uniform(-110, -30, 6)], 1).astype(np.float32)
    lights["bounds"] = np.repeat(rng.uniform(60, 120, 6).astype(np.float32)[:, None], 3, axis=1)
    lights["intensity"] = rng.uniform(40, 250, (6, 3)).astype(np.float32)
    lights["attenuation"] = np.array([1.0, 0.022, 0.0019], np.float32)
    lights["cutOff"] = np.array(host.cutoff_cosines(30.0, 45.0), np.float32)
    lights["direction"] = np.array([0, -1, 0], np.float32)
    lights["type"], lights["shadowType"] = host.LIGHT_POINT, host.SHADOW_PCF
    ibl = synth.make_ibl_set(W, H, oracle.compute_brdf_lut(16, 16), env_size=16, irr_size=8, seed=5, with_ao=True)
    s["ao_in"] = np.ascontiguousarray(ibl.ao, np.float32)
    return cam, s, lights, ibl


def test_one_frame_through_the_shade_against_the_float64_oracle(ctx):
    """resolve_gltf -> sailor_hip_shade_ex with ibl.ao = aoOut -> composite_gltf over a sky-coloured target, 48 x 32, against oracle_f64.shade of the
    RESTATEMENT's planes and aoOut plus the restatement's emissive, under the shade's bound (1e-4 relative + 1e-7 max).  Left out, as in
    the K2 tests of tests/test_ambient_gpu.py and under their cap of 1 %: pixels whose cube direction (normal or Lr) is within 1e-4 of a face seam, where a
    fp32 evaluation may pick the other face.  Uncovered pixels keep the target bit for bit."""
    cam, s, lights, ibl = end_to_end_scene()
    W, H, N = s["W"], s["H"], len(lights)
    want = gltf_ref.render(s)
    c, g = want["covered"], want["gltf"]
    assert 0.3 < c.mean() < 1.0 and (g == c).all() and (want["cutout"] & c).sum() > 10
    assert np.unique(want["ao_out"][c]).size > 50 and (want["ao_out"][c] < s["ao_in"][c]).sum() > 50 and (want["ao_out"][c] == s["ao_in"][c]).sum() > 50
    got = run(ctx, s)
    assert_same(got, want, "the frame")
    lin = linearize_depth(ctx, cam.frame, torch.from_numpy(got["depth"]).to(ctx.device))
    fp = ForwardPlus(ctx, W, H, N)
    d_lights = upload_lights(lights, ctx.device)
    fp.cull(cam.frame, d_lights, N, lin)
    desc, keep = upload_ibl(ibl, ctx.device)
    desc.ao = got["d_ao_out"].data_ptr()
    rad = torch.empty((H, W, 4), dtype=torch.float32, device=ctx.device)
    _lib.check(ctx._lib.sailor_hip_shade_ex(ctx.handle, C.byref(cam.frame), got["surface"].data_ptr(), H * W, d_lights.data_ptr(), N, fp.grid.data_ptr(),
                                            fp.culled.data_ptr(), None, C.byref(desc), rad.data_ptr(), C.byref(fp.band), None), "sailor_hip_shade_ex", ctx.handle)
    sky = np.random.default_rng(3).uniform(0, 1, (H, W, 4)).astype(np.float32)
    main = got["sp"].composite_gltf(rad, got["d_emissive"], dev(ctx, sky)).cpu().numpy()
    ctx.synchronize()
    # the reference side: restatement -> float64 oracle, its ambient term under the restatement's aoOut, plus the restatement's emissive
    og, oi, _ = oracle.light_cull(cam.frame, W, H, lights, oracle.linearize_depth(cam.frame.cameraZNearZFar[0], want["depth"]))
    f64_ibl = dict(irradiance=ibl.irradiance, env_chain=ibl.env_chain, env_size=ibl.env_size, env_levels=ibl.env_levels, brdf_lut=ibl.brdf_lut, ao=want["ao_out"])
    orad, m_n, m_lr = oracle_f64.shade(bytes(cam.frame), W, H, want["planes"], lights, og, oi, None, ibl=f64_ibl, want_seam_margin=True)
    expect = orad[..., :3] + want["emissive"][..., :3].astype(np.float64)
    out = c & ((m_n < 1e-4) | (m_lr < 1e-4))
    print(f"[gltf frame] {c.sum()} covered pixels, {out.sum()} left out for a cube seam: {np.argwhere(out).tolist()}")
    assert out.sum() <= 0.01 * c.size
    keep_px = c & ~out
    err = np.abs(main[..., :3].astype(np.float64) - expect)
    tol = 1e-4 * np.abs(expect) + 1e-7 * np.abs(expect[c]).max()
    print(f"[gltf frame] worst err / tol {(err / tol)[keep_px].max():.3f}; emissive share of the brightest pixel {want['emissive'][..., :3][c].max() / expect[c].max():.3f}")
    assert (err[keep_px] <= tol[keep_px]).all(), f"{(err > tol)[keep_px].sum()} channels beyond the K2 bound"
    assert want["emissive"][..., :3][c].max() > 0.05 and orad[c][:, :3].max() > 0.05, "lit and emissive"
    np.testing.assert_array_equal(main[c][:, 3], orad[c][:, 3].astype(np.float32))
    np.testing.assert_array_equal(main[~c].view(np.uint32), sky[~c].view(np.uint32))
    # aoOut reaches the ambient term: shading with the bound aoIn instead moves pixels beyond the bound
    f64_ibl["ao"] = s["ao_in"]
    other = oracle_f64.shade(bytes(cam.frame), W, H, want["planes"], lights, og, oi, None, ibl=f64_ibl)[..., :3] + want["emissive"][..., :3]
    assert (np.abs(other - expect) > tol)[keep_px].any(), "the occlusion texture does not reach the ambient term in this frame"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_say_why(ctx, scenes):
    lib = ctx._lib
    s = scenes["cutoff_half_is_the_standard_masked_draw"]
    W, H = s["W"], s["H"]
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, W, H, max_draws=2)
    sp.begin()
    ws, n = sp.workspace.data_ptr(), sp.workspace.numel()
    band, frame = sp.band, up.frame
    d = up.draws[1]
    bad_band = _lib.Band(0, 1, 3, 16)
    CUT, GLTF, CULL = _lib.SURFACE_ALPHA_CUTOUT, _lib.SURFACE_GLTF, _lib.SURFACE_CULL_BACK
    surface = torch.empty((3, H, W, 4), dtype=torch.float32, device=ctx.device)
    plane = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    ao = torch.ones(H * W + 1, dtype=torch.float32, device=ctx.device)

    def desc(flags=CUT | GLTF, vertices=d["vertices"].data_ptr(), prim_base=0):
        return _lib.SurfaceDraw(vertices, d["indices"].data_ptr(), d["instance_ids"].data_ptr(), 2, 1, prim_base, flags, 0, 0)

    def draw_call(dd, index=0, workspace=ws, size=n, b=band, inst=up.instances.data_ptr(), mats=up.materials.data_ptr(), nm=2, tex=up.textures.data_ptr(), ntex=up.num_textures,
                  entry=lib.sailor_hip_surface_draw_gltf):
        return lambda: entry(ctx.handle, C.byref(frame), C.byref(dd), inst, mats, nm, tex, ntex, index, W, H, C.byref(b), workspace, size)

    def resolve_call(workspace=ws, size=n, b=band, out=surface.data_ptr(), stride=H * W, mats=up.materials.data_ptr(), tex=up.textures.data_ptr(), inst=up.instances.data_ptr(),
                     ao_in=ao.data_ptr(), ao_out=ao.data_ptr(), em=plane.data_ptr(), depth=None):
        return lambda: lib.sailor_hip_surface_resolve_gltf(ctx.handle, C.byref(frame), inst, mats, 2, tex, up.num_textures, W, H, C.byref(b), workspace, size, out, stride,
                                                           depth, None, ao_in, ao_out, em)

    def composite_call(rad=plane.data_ptr(), em=plane.data_ptr(), workspace=ws, size=n, tgt=plane.data_ptr(), b=band):
        return lambda: lib.sailor_hip_surface_composite_gltf(ctx.handle, rad, em, workspace, size, tgt, W, H, C.byref(b))
    misuse = {
        "draw_gltf: without the glTF flag": draw_call(desc(flags=CUT)),
        "draw_gltf: no flag at all": draw_call(desc(flags=0)),
        "draw_gltf: unknown flag bits": draw_call(desc(flags=GLTF | 8)),
        "draw_gltf: the cutout flag with null materials": draw_call(desc(), mats=None),
        "draw_gltf: the cutout flag with null textures": draw_call(desc(), tex=None),
        "draw_gltf: the cutout flag with no materials": draw_call(desc(), nm=0),
        "draw_gltf: the cutout flag with no textures": draw_call(desc(), ntex=0),
        "draw_gltf: null vertices": draw_call(desc(vertices=None)),
        "draw_gltf: null instances": draw_call(desc(), inst=None),
        "draw_gltf: null workspace": draw_call(desc(), workspace=None),
        "draw_gltf: workspace too small": draw_call(desc(), size=1000),
        "draw_gltf: drawIndex >= maxDraws": draw_call(desc(), index=2),
        "draw_gltf: primBase overflow": draw_call(desc(prim_base=2 ** 32 - 1 - 4)),
        "draw_gltf: invalid band": draw_call(desc(), b=bad_band),
        "draw_masked: the glTF flag": draw_call(desc(flags=CUT | GLTF), entry=lib.sailor_hip_surface_draw_masked),
        "draw_masked: the glTF flag alone": draw_call(desc(flags=GLTF), entry=lib.sailor_hip_surface_draw_masked),
        "draw: the glTF flag": lambda: lib.sailor_hip_surface_draw(ctx.handle, C.byref(frame), C.byref(desc(flags=GLTF)), up.instances.data_ptr(), 0, W, H, C.byref(band), ws, n),
        "resolve_gltf: null surface": resolve_call(out=None),
        "resolve_gltf: null materials": resolve_call(mats=None),
        "resolve_gltf: null textures": resolve_call(tex=None),
        "resolve_gltf: null instances": resolve_call(inst=None),
        "resolve_gltf: planeStride too small": resolve_call(stride=H * W - 1),
        "resolve_gltf: workspace too small": resolve_call(size=1000),
        "resolve_gltf: null workspace": resolve_call(workspace=None),
        "resolve_gltf: invalid band": resolve_call(b=bad_band),
        "resolve_gltf: null emissive": resolve_call(em=None),
        "resolve_gltf: misaligned emissive": resolve_call(em=plane.data_ptr() + 4),
        "resolve_gltf: misaligned aoIn": resolve_call(ao_in=ao.data_ptr() + 2),
        "resolve_gltf: misaligned aoOut": resolve_call(ao_out=ao.data_ptr() + 2),
        "resolve_gltf: misaligned depth": resolve_call(depth=ao.data_ptr() + 2),
        "composite_gltf: null radiance": composite_call(rad=None),
        "composite_gltf: null emissive": composite_call(em=None),
        "composite_gltf: null target": composite_call(tgt=None),
        "composite_gltf: misaligned emissive": composite_call(em=plane.data_ptr() + 4),
        "composite_gltf: null workspace": composite_call(workspace=None),
        "composite_gltf: workspace too small": composite_call(size=1000),
        "composite_gltf: invalid band": composite_call(b=bad_band),
    }
    for what, call in misuse.items():
        before, _ = ctx.launch_log(0)
        assert call() == -1, what
        after, _ = ctx.launch_log(0)
        assert after == before, f"{what}: launched {after - before} kernels"
        assert b"sailor_hip_surface_" in lib.sailor_hip_context_last_error(ctx.handle), what
    last = lambda call: (call(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"does not carry SAILOR_SURFACE_GLTF" in last(draw_call(desc(flags=CUT)))
    assert b"ALPHA_CUTOUT needs materials and textures" in last(draw_call(desc(), mats=None))
    assert b"draw_gltf: unknown flags" in last(draw_call(desc(flags=GLTF | 8)))
    assert b"draw_masked: unknown flags" in last(draw_call(desc(flags=CUT | GLTF), entry=lib.sailor_hip_surface_draw_masked))
    assert b"emissive" in last(resolve_call(em=None)) and b"occlusion plane" in last(resolve_call(ao_in=ao.data_ptr() + 2))
    # without the cutout flag the tables may be absent; every legal flag combination; the largest primBase still accepted; aoIn, aoOut and depth may be NULL
    assert draw_call(desc(flags=GLTF), mats=None, nm=0, tex=None, ntex=0)() == 0
    assert draw_call(desc(flags=GLTF | CUT | CULL, prim_base=2 ** 32 - 2 - 4), index=1)() == 0
    assert resolve_call(ao_in=None, ao_out=None)() == 0
    ctx.synchronize()
    names = ctx.launches_of(lambda: (sp.begin(), up.draw_all(sp), sp.resolve_gltf(frame, up.instances, up.materials, up.textures, up.num_textures),
                                     sp.composite_gltf(plane.clone(), plane.clone(), plane)))
    assert names == ["k_surface_begin", "k_surface_visibility", "k_surface_visibility_gltf", "k_surface_resolve_gltf", "k_surface_composite_gltf"], names
    ctx.synchronize()


# ---- timing -------------------------------------------------------------------------------------------------------------------------------------------
def test_launch_times_at_4k(ctx):
    """prints the per-launch medians at 3840 x 2160 on surface_cases.boxes_and_ground (1 024 boxes and a ground quad behind their depth prepass): the existing
    kernels on the Standard scene and, in the same run, the glTF kernels on the same scene with every draw flagged glTF (opaque, and with ALPHA_CUTOUT).  No
    assertion on a value: these kernels have no parent to compare against."""
    W, H = 3840, 2160
    s = surface_cases.boxes_and_ground(1024, W, H)
    g = cases.as_gltf(s)
    variants = {"standard": s, "gltf": g, "gltf cutout": dict(g, draws=[cases.cutout(d) for d in g["draws"]])}
    lib = ctx._lib
    up0 = Uploaded(ctx, s)
    models = dev(ctx, np.ascontiguousarray(s["instances"]["model"]))
    raw = torch.zeros((H, W), dtype=torch.float32, device=ctx.device)
    keep = []
    for d in s["draws"]:
        pos, idx = dev(ctx, np.ascontiguousarray(d["vertices"][:, 2:5])), dev(ctx, d["indices"], np.int32)
        dids = dev(ctx, np.arange(d["first_instance"], d["first_instance"] + d["num_drawn"], dtype=np.uint32), np.int32)
        keep += [pos, idx, dids]
        _lib.check(lib.sailor_hip_raster_depth_camera(ctx.handle, C.byref(up0.frame), pos.data_ptr(), idx.data_ptr(), len(d["indices"]), models.data_ptr(), dids.data_ptr(),
                                                      d["num_drawn"], W, H, raw.data_ptr(), _lib.RASTER_CULL_BACK if d["cull_back"] else 0, None), "prepass", ctx.handle)
    sp = SurfacePass(ctx, W, H)
    radiance = torch.rand((H, W, 4), dtype=torch.float32, device=ctx.device)
    target = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
    ao = torch.rand((H, W), dtype=torch.float32, device=ctx.device)
    for label, scene in variants.items():
        up = Uploaded(ctx, scene)
        is_gltf = label != "standard"
        times = {"begin": [], "draw boxes": [], "draw ground": [], "resolve": [], "composite": []}
        for it in range(7):
            ctx.time_launches(0, 5)
            sp.begin(raw)
            up.draw_all(sp)
            if is_gltf:
                surface, depth, cov, ao_out, emissive = sp.resolve_gltf(up.frame, up.instances, up.materials, up.textures, up.num_textures, ao_in=ao)
                sp.composite_gltf(radiance, emissive, target)
            else:
                surface, depth, cov = sp.resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures)
                sp.composite(radiance, target)
            ctx.synchronize()
            if it >= 2:
                for slot, key in enumerate(times):
                    times[key].append(ctx.timed_launch_ms(slot))
        covered = float(cov.float().mean())
        if label != "gltf cutout":
            np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), raw.cpu().numpy().view(np.uint32))
        for key, v in times.items():
            print(f"[{label}] surface launch {key} 3840x2160: median {np.median(v) * 1e3:.1f} us (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}, n={len(v)})")
        print(f"[{label}] {covered:.3f} of the frame covered")
        assert all(len(v) == 5 for v in times.values()) and (covered > 0.3 or label == "gltf cutout")
        del surface, depth, cov
    floor = W * H * (8 + 48 + 4 + 1 + 4 + 4 + 16)   # resolve_gltf reads a key and an aoIn and writes three float4, a depth, a coverage byte, aoOut and emissive per pixel
    print(f"resolve_gltf 3840x2160: byte floor {floor / 1e6:.1f} MB = {floor / 6.29e12 * 1e6:.1f} us at 6.29 TB/s")
