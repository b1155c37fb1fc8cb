"""Mip-mapped material textures on the device (sailor_amd/csrc/texture_mips.hip, surface_lod.hip) through the C-ABI: the generated chains byte for byte against
tests/lod_ref.py; the `_lod` entry points over one-level tables against the existing entry points on every scene of the surface, masked, glTF and indirect
suites, bit for bit; the cases of tests/lod_cases.py with chains against the restatement -- keys, depth and coverage bit for bit, planes, emissive and ao bit
for bit with non-finite words compared by class --, in bands of a world of 2 and of 3; the known answers of tests/test_lod_cpu.py; the refusals of the
generation; and the resolve's launch time at 3840 x 2160 with and without chains (printed, nothing asserted)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gltf_cases
import indirect_cases
import lod_cases as cases
import lod_ref
import masked_cases
import surface_cases
import surface_ref as ref
from sailor_amd import _lib, host
from sailor_amd.forward_plus import SurfacePass, upload_textures
from test_indirect_gpu import commands_of
from test_lod_cpu import check_known_answers
from test_surface_gpu import dev, frame_of

pytestmark = pytest.mark.gpu


def upload_chains(ctx, s):
    """the scene's texture table with its chains behind the descriptors (level 0 alone without chains), the `levels` fields as the scene writes them; an image
    of shape (0, 0, 4) is a descriptor without texels"""
    n = len(s["textures"])
    chains, fields = s.get("chains") or [None] * n, s.get("levels")
    keep, table = [], (_lib.TextureDesc * n)()
    for k, (img, g) in enumerate(zip(s["textures"], s["srgb"])):
        img = np.ascontiguousarray(img, np.uint8)
        if img.shape[0] == 0 or img.shape[1] == 0:
            table[k] = _lib.TextureDesc(None, 0, 0, 0, 0)
            continue
        chain = [img] if chains[k] is None else chains[k]
        t = dev(ctx, lod_ref.flat_chain(chain), np.int32)
        keep.append(t)
        table[k] = _lib.TextureDesc(t.data_ptr(), img.shape[1], img.shape[0], _lib.TEXTURE_SRGB if g else 0, 0 if fields is None else int(fields[k]))
    d = torch.from_numpy(np.frombuffer(bytes(table), np.uint8).copy()).to(ctx.device)
    return d, n, keep + [d]


class Uploaded:
    """a scene's buffers on the device: direct and indirect draws, Standard and glTF, with or without chains"""

    def __init__(self, ctx, s, textures=None):
        self.s, self.frame = s, frame_of(s)
        self.instances = dev(ctx, s["instances"].view(np.uint8))
        self.materials = dev(ctx, s["materials"].view(np.uint8))
        self.textures, self.num_textures, self.keep = textures or upload_chains(ctx, s)
        spare = torch.zeros(3, dtype=torch.int32, device=ctx.device)
        self.draws = [dict(vertices=dev(ctx, d["vertices"]), indices=dev(ctx, d["indices"], np.int32) if len(d["indices"]) else spare[:0]) for d in s["draws"]]
        self.ids = [None if d.get("instance_ids") is None else dev(ctx, d["instance_ids"], np.int32) for d in s["draws"]]
        self.commands = dev(ctx, commands_of(s), np.int32) if any(d.get("indirect") is not None for d in s["draws"]) else None
        self.ao_in = None if s.get("ao_in") is None else np.asarray(s["ao_in"], np.float32)

    def draw_all(self, sp, lod):
        k = 0
        for d, u, ids in zip(self.s["draws"], self.draws, self.ids):
            cut, gltf = bool(d.get("alpha_cutout", False)), bool(d.get("gltf", False))
            tables = dict(materials=self.materials, textures=self.textures, num_textures=self.num_textures) if cut or gltf else {}
            ind = d.get("indirect")
            if ind is None:
                sp.draw(self.frame, instances=self.instances, instance_ids=ids, num_drawn=d["num_drawn"], first_instance=d["first_instance"], cull_back=d["cull_back"],
                        alpha_cutout=cut, gltf=gltf, lod=lod, **tables, **u)
            else:
                sp.draw_indirect(self.frame, instances=self.instances, command=self.commands, command_index=k, capacity=ind["capacity"],
                                 num_instance_records=self.s["records"] if ind.get("records") is None else ind["records"], cull_back=d["cull_back"],
                                 alpha_cutout=cut, gltf=gltf, lod=lod, **tables, **u)
                k += 1


def run(ctx, s, lod=True, prepass=None, band=None, up=None):
    """the scene through begin / the draws / the resolve -> dict like lod_ref.render's.  lod: the `_lod` entry points, otherwise the existing ones"""
    up = up or Uploaded(ctx, s)
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=max(len(s["draws"]), 1))
    sp.begin(None if prepass is None else dev(ctx, prepass), prim_base=s.get("prim_base", 0))
    up.draw_all(sp, lod)
    rows = slice(sp.band.fbRowBegin, sp.band.fbRowBegin + sp.band.fbRowCount)
    d_ao = None if up.ao_in is None else dev(ctx, up.ao_in[rows])
    resolve = sp.resolve_lod if lod else sp.resolve_gltf
    surface, depth, cov, ao_out, emissive = resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures, ao_in=d_ao)
    return dict(planes=surface.cpu().numpy(), depth=depth.cpu().numpy(), covered=cov.cpu().numpy().astype(bool), keys=sp.download_keys(), ao_out=ao_out.cpu().numpy(),
                emissive=emissive.cpu().numpy(), sp=sp, up=up)


def assert_same(got, want, what=""):
    np.testing.assert_array_equal(got["keys"], want["keys"], err_msg=f"{what}: keys")
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), err_msg=f"{what}: depth")
    np.testing.assert_array_equal(got["covered"], want["covered"], err_msg=f"{what}: coverage")
    for k in ("planes", "emissive", "ao_out"):
        same = ref.same_bits_or_class(got[k], want[k])
        assert same.all(), f"{what}: {(~same).sum()} words of {k} differ, first at {np.argwhere(~same)[:4].tolist()}"


# ---- 1. the chain -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_generated_chains_are_the_restatements_byte_for_byte(ctx, srgb):
    images = [cases.random_texture(w, h, 50 + k) for k, (w, h) in enumerate(cases.EXTENTS)]
    images[0][:2, :2] = [[[0, 0, 0, 0], [255, 255, 255, 255]], [[1, 254, 127, 128], [2, 3, 253, 1]]]      # the ends of the tables
    table, n, keep = upload_textures(ctx, images, [srgb] * len(images), mips=True)
    ctx.synchronize()
    descs = table.cpu().numpy().view(np.uint32).reshape(n, 6)
    for k, img in enumerate(images):
        h, w = img.shape[:2]
        want = lod_ref.flat_chain(lod_ref.build_chain(img, srgb))
        got = keep[k].cpu().numpy().view(np.uint32)
        assert descs[k, 5] == lod_ref.full_levels(w, h) and descs[k, 4] == (1 if srgb else 0) and (descs[k, 2], descs[k, 3]) == (w, h)
        assert got.size == want.size == host.mip_chain_texels(w, h, lod_ref.full_levels(w, h))
        differ = np.nonzero(got != want)[0]
        assert differ.size == 0, f"{w} x {h}: {differ.size} texels differ, first at {differ[:4].tolist()}: {got[differ[:4]]} != {want[differ[:4]]}"
    names = ctx.launches_of(lambda: upload_textures(ctx, images[-1:], [srgb], mips=True))
    assert names == ["k_texture_mip_down"] * 6, names
    ctx.synchronize()


def test_fewer_levels_leave_the_rest_untouched_and_refusals_launch_nothing(ctx):
    lib = ctx._lib
    img = cases.random_texture(17, 9, 3)
    flat = np.full(host.mip_chain_texels(17, 9, 5), 0xDEADBEEF, np.uint32)
    flat[: 17 * 9] = img.view(np.uint32).reshape(-1)
    t = dev(ctx, flat, np.int32)
    assert lib.sailor_hip_texture_generate_mips(ctx.handle, t.data_ptr(), 17, 9, 3, _lib.TEXTURE_SRGB) == 0
    ctx.synchronize()
    got = t.cpu().numpy().view(np.uint32)
    want = lod_ref.flat_chain(lod_ref.build_chain(img, True, levels=3))
    assert np.array_equal(got[: want.size], want) and (got[want.size:] == 0xDEADBEEF).all()
    misuse = {"null texels": (None, 17, 9, 3, 0), "misaligned texels": (t.data_ptr() + 2, 17, 9, 3, 0), "zero width": (t.data_ptr(), 0, 9, 1, 0),
              "height beyond 32768": (t.data_ptr(), 17, 32769, 1, 0), "no level": (t.data_ptr(), 17, 9, 0, 0), "more levels than the chain has": (t.data_ptr(), 17, 9, 6, 0),
              "unknown flags": (t.data_ptr(), 17, 9, 3, 2)}
    for what, args in misuse.items():
        before, _ = ctx.launch_log(0)
        assert lib.sailor_hip_texture_generate_mips(ctx.handle, *args) == -1, what
        assert ctx.launch_log(0)[0] == before, what
        assert b"sailor_hip_texture_generate_mips" in lib.sailor_hip_context_last_error(ctx.handle), what
    assert lib.sailor_hip_texture_generate_mips(ctx.handle, t.data_ptr(), 17, 9, 1, 0) == 0      # one level: nothing to do
    ctx.synchronize()


# ---- 2. one-level tables through the `_lod` entry points ---------------------------------------------------------------------------------------------------
def _family(which):
    if which == "surface":
        return {name: build() for name, (build, _) in surface_cases.CASES.items()}
    if which == "masked":
        return masked_cases.all_scenes()
    if which == "gltf":
        return gltf_cases.all_scenes()
    return indirect_cases.all_scenes()


@pytest.mark.parametrize("which", ["surface", "masked", "gltf", "indirect"])
def test_one_level_tables_give_the_existing_entry_points_bits(ctx, which):
    scenes = _family(which)
    assert len(scenes) >= 15
    for name, s in scenes.items():
        up = Uploaded(ctx, s)
        assert_same(run(ctx, s, lod=True, up=up), run(ctx, s, lod=False, up=up), f"{which} {name}")
    ctx.synchronize()


# ---- 3. the cases with chains ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.fixture(scope="module")
def rendered(scenes):
    return {name: lod_ref.render(s) for name, s in scenes.items()}   # computed once, shared, left unchanged


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_with_chains_against_the_restatement(ctx, scenes, rendered, name):
    s, want = scenes[name], rendered[name]
    got = run(ctx, s)
    assert_same(got, want, name)
    own = want["cutout"] & want["covered"]
    if own.any():       # every pixel a cutout draw owns holds, bit for bit, the alpha that was tested: not below its threshold
        np.testing.assert_array_equal(got["planes"][0][own][:, 3].view(np.uint32), want["stats"]["alpha"][own].view(np.uint32))
        assert (got["planes"][0][own][:, 3] >= want["stats"]["threshold"][own]).all()
    launched = ctx.launches_of(lambda: run(ctx, s, up=got["up"]))
    assert launched[-1] == "k_surface_resolve_lod" and all("_lod" in k for k in launched[1:]), launched
    ctx.synchronize()


def test_device_made_chains_give_the_same_frame(ctx, scenes, rendered):
    """upload_textures(mips=True): level 0 up, the chain generated on the device, the descriptor's levels set -- the frame is the restatement's"""
    for name in ("receding_ground", "mixed_pass"):
        s = scenes[name]
        assert_same(run(ctx, s, up=Uploaded(ctx, s, textures=upload_textures(ctx, s["textures"], s["srgb"], mips=True))), rendered[name], name)


def test_a_prepass_and_back_face_culling(ctx, scenes):
    for name in ("receding_ground", "cutout_per_level", "near_cut"):
        s = scenes[name]
        pre = lod_ref.render(s)["depth"]
        assert_same(run(ctx, s, prepass=pre), lod_ref.render(s, prepass=pre), f"{name} behind its own depth")
        c = surface_cases.with_cull_back(s)
        assert_same(run(ctx, c), lod_ref.render(c), f"{name} with back-face culling")


# ---- 4. bands ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_bands_concatenate_to_the_whole_frame(ctx, scenes, rendered, world):
    for name in cases.BAND_CASES:
        s, whole = scenes[name], rendered[name]
        up, parts = Uploaded(ctx, s), []
        for rank in reversed(range(world)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
            band = host.band_for_rank(s["W"], s["H"], rank, world)
            if band.fbRowCount == 0:
                continue
            got = run(ctx, s, band=band, up=up)
            assert_same(got, lod_ref.render(s, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)), f"{name} band {rank}/{world}")
            parts.append(got)
        assert len(parts) >= 2
        np.testing.assert_array_equal(np.concatenate([p["keys"] for p in parts]), whole["keys"])
        for k, axis in (("planes", 1), ("emissive", 0), ("ao_out", 0)):
            assert ref.same_bits_or_class(np.concatenate([p[k] for p in parts], axis=axis), whole[k]).all(), (name, k)


# ---- 5. known answers --------------------------------------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_device(ctx):
    check_known_answers(lambda s: run(ctx, s))


# ---- 7. timing ---------------------------------------------------------------------------------------------------------------------------------------------
def test_resolve_launch_times_at_4k(ctx):
    """prints k_surface_resolve_gltf on one-level tables against k_surface_resolve_lod on chains at 3840 x 2160: a ground plane under 2048 x 2048 textures,
    the two alternated, 20 event-timed launches each after a warm-up, median and p10 / p90.  Asserts nothing about a value."""
    W, H, N = 3840, 2160, 2048
    p = [(-1.5, -0.5, -1.0), (1.5, -0.5, -1.0), (36.0, 8.0, -30.0), (-36.0, 8.0, -30.0)]
    v = [surface_cases.vertex(q, (q[0] * 0.5, q[2] * 0.5)) for q in p]
    rng = np.random.default_rng(1)
    images = [rng.integers(0, 256, (N, N, 4), dtype=np.uint8) for _ in range(3)]
    s = surface_cases.scene(W, H, surface_cases.camera_projection(W, H), [surface_cases.draw(v, [(0, 1, 2), (0, 2, 3)])], textures=images, srgb=[True, False, True],
                            mats=[surface_cases.material(samplers=(0, 2, 1, 2))])
    flat = Uploaded(ctx, s, textures=upload_textures(ctx, images, s["srgb"]))
    chains = Uploaded(ctx, s, textures=upload_textures(ctx, images, s["srgb"], mips=True))
    sp = SurfacePass(ctx, W, H)
    sp.begin()
    flat.draw_all(sp, lod=False)
    times = {"k_surface_resolve_gltf, one level": [], "k_surface_resolve_lod, chains": []}
    for it in range(23):
        for (label, up, resolve) in (("k_surface_resolve_gltf, one level", flat, sp.resolve_gltf), ("k_surface_resolve_lod, chains", chains, sp.resolve_lod)):
            ctx.time_launches(0, 1)
            out = resolve(up.frame, up.instances, up.materials, up.textures, up.num_textures)
            ctx.synchronize()
            if it >= 3:
                times[label].append(ctx.timed_launch_ms(0))
            covered = float(out[2].float().mean())
            del out
    for label, t in times.items():
        print(f"[lod 4k] {label}: median {np.median(t) * 1e3:.1f} us, p10 {np.percentile(t, 10) * 1e3:.1f}, p90 {np.percentile(t, 90) * 1e3:.1f} (n={len(t)}); "
              f"{covered:.3f} of the frame covered")
    assert all(len(t) == 20 for t in times.values())
