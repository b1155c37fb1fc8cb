"""The indirect surface draw (sailor_amd/csrc/surface_indirect.hip) through the C-ABI: every case of tests/indirect_cases.py against the existing
restatements run on the survivors (tests/indirect_ref.py) -- keys decoded to (slot, d, triangle, part) with each side's own primBase table plus the depth bits;
planes, depth and coverage (and, for glTF passes, emissive and aoOut) raw, bit for bit --, behind a prepass and in two bands; the refusals; the chain
MeshCull.run -> draw_indirect on one stream with no download in between, frustum only and with the Hi-Z pyramid of a wall; and the chain captured once and
replayed over two sets of instance records."""
import ctypes as C

import numpy as np
import pytest
import torch

import indirect_cases as cases
import indirect_ref as iref
import surface_ref as ref
from oracle import oracle
from sailor_amd import _lib, host
from sailor_amd.forward_plus import HipContext, MeshCull, SurfacePass, hiz_build
from test_masked_gpu import upload_textures
from test_surface_gpu import dev, frame_of

pytestmark = pytest.mark.gpu


def commands_of(s):
    """the scene's indirect commands as the 20-byte records the draws read: (indexCount, instanceCount, firstIndex, vertexOffset, firstInstance)"""
    rows = [(3 * len(d["indices"]), d["indirect"]["count"], 0, 0, d["indirect"]["first"]) for d in s["draws"] if d.get("indirect") is not None]
    return np.array(rows, np.uint32).reshape(-1, 5)


class Uploaded:
    """a scene's buffers on the device; the instance buffer WITH its slack, the commands in one buffer"""

    def __init__(self, ctx, s):
        self.s, self.frame = s, frame_of(s)
        self.instances = dev(ctx, s["instances"].view(np.uint8))
        self.materials = dev(ctx, s["materials"].view(np.uint8))
        self.textures, self.num_textures, self.keep = upload_textures(ctx, s["textures"], s["srgb"])
        self.draws = [dict(vertices=dev(ctx, d["vertices"]), indices=dev(ctx, d["indices"], np.int32)) for d in s["draws"]]
        self.ids = [None if d.get("instance_ids") is None else dev(ctx, d["instance_ids"], np.int32) for d in s["draws"]]
        self.commands = dev(ctx, commands_of(s), np.int32)
        self.gltf = any(d.get("gltf", False) for d in s["draws"])

    def draw_all(self, sp, instances=None, commands=None):
        instances = self.instances if instances is None else instances
        commands = self.commands if commands is None else commands
        k = 0
        for d, u, ids in zip(self.s["draws"], self.draws, self.ids):
            cut, gltf = bool(d.get("alpha_cutout", False)), bool(d.get("gltf", False))
            tables = dict(materials=self.materials, textures=self.textures, num_textures=self.num_textures) if cut or gltf else {}
            ind = d.get("indirect")
            if ind is None:
                sp.draw(self.frame, instances=instances, instance_ids=ids, num_drawn=d["num_drawn"], first_instance=d["first_instance"], cull_back=d["cull_back"],
                        alpha_cutout=cut, gltf=gltf, **tables, **u)
            else:
                sp.draw_indirect(self.frame, instances=instances, command=commands, command_index=k, capacity=ind["capacity"],
                                 num_instance_records=self.s["records"] if ind.get("records") is None else ind["records"], cull_back=d["cull_back"],
                                 alpha_cutout=cut, gltf=gltf, **tables, **u)
                k += 1

    def resolve(self, sp, instances=None):
        instances = self.instances if instances is None else instances
        if self.gltf:
            surface, depth, cov, ao_out, emissive = sp.resolve_gltf(self.frame, instances, self.materials, self.textures, self.num_textures)
            return dict(surface=surface, depth=depth, cov=cov, ao_out=ao_out, emissive=emissive)
        surface, depth, cov = sp.resolve(self.frame, instances, self.materials, self.textures, self.num_textures)
        return dict(surface=surface, depth=depth, cov=cov)


def downloaded(sp, out):
    got = dict(keys=sp.download_keys(), planes=out["surface"].cpu().numpy(), depth=out["depth"].cpu().numpy(), covered=out["cov"].cpu().numpy().astype(bool))
    for k in ("emissive", "ao_out"):
        if k in out:
            got[k] = out[k].cpu().numpy()
    return got


def run(ctx, s, prepass=None, band=None, up=None):
    up = up or Uploaded(ctx, s)
    sp = SurfacePass(ctx, s["W"], s["H"], band, max_draws=max(len(s["draws"]), 1))
    sp.begin(None if prepass is None else dev(ctx, prepass), prim_base=s.get("prim_base", 0))
    up.draw_all(sp)
    return dict(downloaded(sp, up.resolve(sp)), sp=sp, up=up)


def assert_same(got, want, s, what=""):
    """got: the indirect pass of scene s on the device; want: the existing restatement on the survivors"""
    mine, theirs = iref.decode(got["keys"], iref.prim_table(s, "capacity")), iref.decode(want["keys"], iref.prim_table(s, "survivors"))
    for k in ("slot", "d", "triangle", "part", "depth"):
        np.testing.assert_array_equal(mine[k], theirs[k], err_msg=f"{what}: the keys' {k}")
    np.testing.assert_array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), err_msg=f"{what}: depth")
    np.testing.assert_array_equal(got["covered"], want["covered"], err_msg=f"{what}: coverage")
    for k in ("planes", "emissive", "ao_out"):
        if k in want and k in got:
            same = ref.same_bits_or_class(got[k], want[k])
            assert same.all(), f"{what}: {(~same).sum()} words of {k} differ, first at {np.argwhere(~same)[:4].tolist()}"
    assert ("emissive" in got) == ("emissive" in want), what


@pytest.fixture(scope="module")
def scenes():
    return cases.all_scenes()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_case_against_the_restatement_of_the_survivors_with_and_without_a_prepass(ctx, scenes, name):
    s = scenes[name]
    up = Uploaded(ctx, s)
    got = run(ctx, s, up=up)
    assert_same(got, iref.expected(s), s, name)
    np.testing.assert_array_equal(got["keys"], iref.render_keys(s), err_msg=f"{name}: the raw keys, low words by the capacity")
    pre = cases.prepass(iref.survivors(s))
    assert_same(run(ctx, s, prepass=pre, up=up), iref.expected(s, prepass=pre), s, f"{name} behind its prepass")
    # the descriptors the draws left: numDrawn = n and firstInstance as read (rule 4), in the slots' order
    sp = got["sp"]
    at = ctx._lib.sailor_hip_surface_keys_offset() + sp.rows * sp.W * 8
    slots = sp.workspace[at: at + 48 * len(s["draws"])].cpu().numpy().view(np.uint32).reshape(-1, 12)
    for k, (d, (base, _, nt, n)) in enumerate(zip(s["draws"], iref.prim_table(s, "capacity"))):
        assert (slots[k, 6], slots[k, 7], slots[k, 8]) == (nt, n, base), (name, k, slots[k])
        if d.get("indirect") is not None:
            assert slots[k, 10] == d["indirect"]["first"] and slots[k, 4] == 0 and slots[k, 5] == 0, (name, k, slots[k])


def test_two_bands_concatenate_to_the_whole_frame(ctx, scenes):
    for name in cases.BAND_CASES:
        s = scenes[name]
        up, parts = Uploaded(ctx, s), []
        for rank in reversed(range(2)):   # tile row 0 is the BOTTOM of the framebuffer: the last rank's band holds the first rows
            band = host.band_for_rank(s["W"], s["H"], rank, 2)
            got = run(ctx, s, band=band, up=up)
            assert_same(got, iref.expected(s, rows=(band.fbRowBegin, band.fbRowBegin + band.fbRowCount)), s, f"{name} band {rank}/2")
            parts.append(got)
        whole = dict(keys=np.concatenate([p["keys"] for p in parts]), depth=np.concatenate([p["depth"] for p in parts]),
                     covered=np.concatenate([p["covered"] for p in parts]), planes=np.concatenate([p["planes"] for p in parts], axis=1))
        want = iref.expected(s)
        assert_same(whole, {k: want[k] for k in ("keys", "depth", "covered", "planes")}, s, f"{name}: the bands together")


def test_the_launches_are_the_indirect_kernels(ctx, scenes):
    for name, kernels in (("boxes_5_of_24", ["k_surface_visibility_indirect"] * 2), ("gltf_partial", ["k_surface_visibility_indirect_gltf"] * 2),
                          ("mixed_direct_and_indirect", ["k_surface_visibility", "k_surface_visibility_indirect", "k_surface_visibility_masked",
                                                         "k_surface_visibility_indirect_gltf", "k_surface_visibility_indirect", "k_surface_visibility"])):
        s = scenes[name]
        up = Uploaded(ctx, s)
        sp = SurfacePass(ctx, s["W"], s["H"], max_draws=len(s["draws"]))
        sp.begin()
        assert ctx.launches_of(lambda: up.draw_all(sp)) == kernels, name
        ctx.synchronize()


def test_refusals_launch_nothing_and_say_why(ctx, scenes):
    lib = ctx._lib
    s = scenes["cutout_partial"]
    Wd, Ht = s["W"], s["H"]
    up = Uploaded(ctx, s)
    sp = SurfacePass(ctx, Wd, Ht, max_draws=2)
    sp.begin()
    ws, n = sp.workspace.data_ptr(), sp.workspace.numel()
    band, frame, d = sp.band, up.frame, up.draws[0]
    bad_band = _lib.Band(0, 1, 3, 16)
    ids = torch.zeros(8, dtype=torch.int32, device=ctx.device)
    CUT, GLTF = _lib.SURFACE_ALPHA_CUTOUT, _lib.SURFACE_GLTF

    def desc(flags=CUT, vertices=d["vertices"].data_ptr(), prim_base=0, instance_ids=None, capacity=6):
        return _lib.SurfaceDraw(vertices, d["indices"].data_ptr(), instance_ids, 2, capacity, prim_base, flags, 0, 0)

    def call(dd, index=0, workspace=ws, size=n, b=band, inst=up.instances.data_ptr(), mats=up.materials.data_ptr(), nm=4, tex=up.textures.data_ptr(), ntex=up.num_textures,
             command=up.commands.data_ptr(), fr=frame):
        return lambda: lib.sailor_hip_surface_draw_indirect(ctx.handle, C.byref(fr) if fr is not None else None, C.byref(dd) if dd is not None else None, command, inst,
                                                            s["records"], mats, nm, tex, ntex, index, Wd, Ht, C.byref(b), workspace, size)
    misuse = {
        "null command": call(desc(), command=None),
        "misaligned command": call(desc(), command=up.commands.data_ptr() + 2),
        "instance ids": call(desc(instance_ids=ids.data_ptr())),
        "null draw": call(None),
        "null frame": call(desc(), fr=None),
        "the flag with null materials": call(desc(), mats=None),
        "the flag with null textures": call(desc(), tex=None),
        "the flag with no materials": call(desc(), nm=0),
        "the flag with no textures": call(desc(), ntex=0),
        "the glTF cutout with null materials": call(desc(flags=CUT | GLTF), mats=None),
        "unknown flag bits": call(desc(flags=CUT | 8)),
        "unknown flag bits alone": call(desc(flags=0x80000000)),
        "null vertices": call(desc(vertices=None)),
        "null instances": call(desc(), inst=None),
        "null workspace": call(desc(), workspace=None),
        "workspace too small": call(desc(), size=1000),
        "drawIndex >= maxDraws": call(desc(), index=2),
        "primBase overflow by the capacity": call(desc(prim_base=2 ** 32 - 1 - 24)),
        "too many lanes": call(desc(capacity=2 ** 31)),
        "invalid band": call(desc(), b=bad_band),
    }
    for what, c in misuse.items():
        before, _ = ctx.launch_log(0)
        assert c() == -1, what
        after, _ = ctx.launch_log(0)
        assert after == before, f"{what}: launched {after - before} kernels"
        assert b"sailor_hip_surface_draw_indirect" in lib.sailor_hip_context_last_error(ctx.handle), what
    assert b"command is NULL or not 4-byte aligned" in (call(desc(), command=None)(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"dInstanceIds must be NULL" in (call(desc(instance_ids=ids.data_ptr()))(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert b"ALPHA_CUTOUT needs materials and textures" in (call(desc(), mats=None)(), lib.sailor_hip_context_last_error(ctx.handle))[1]
    assert lib.sailor_hip_surface_draw_indirect(None, C.byref(frame), C.byref(desc()), up.commands.data_ptr(), up.instances.data_ptr(), s["records"], None, 0, None, 0, 0,
                                                Wd, Ht, C.byref(band), ws, n) == -1
    # without the flag the tables may be absent; the largest primBase still accepted (6 instances x 2 triangles x 2 = 24 orders); a capacity of 0 records
    assert call(desc(flags=0), mats=None, nm=0, tex=None, ntex=0)() == 0
    assert call(desc(prim_base=2 ** 32 - 2 - 24), index=1)() == 0
    assert call(desc(capacity=0), index=1)() == 0
    ctx.synchronize()


# ---- the chain: cull -> draw on one stream -----------------------------------------------------------------------------------------------------------
def chain_pass(c, up, mc, sp, hiz=None):
    """record the cull and compaction, then the pass over what they leave in device memory; nothing is downloaded in between"""
    instances, commands = mc.run(c["frame"], num_instances=c["scene"]["records"], hiz=hiz)
    sp.begin()
    up.draw_all(sp, instances=instances, commands=commands)
    return up.resolve(sp, instances=instances)


def padded_records(s):
    return s["instances"]   # records and slack: the cull is told `records`, the buffer is longer


def test_the_chain_frustum_only(ctx):
    build, counts = cases.CHAINS["chain_frustum"]
    c = build()
    s = c["scene"]
    up = Uploaded(ctx, s)
    mc = MeshCull(ctx, padded_records(s), c["batches"])
    sp = SurfacePass(ctx, s["W"], s["H"], max_draws=len(s["draws"]))
    out = chain_pass(c, up, mc, sp)
    got = downloaded(sp, out)
    after, want_counts = cases.chain_after_cull(c)
    assert want_counts == counts
    assert_same(got, iref.expected(after), after, "the chain against direct draws of the oracle's survivors")
    _, batches = mc.download()
    assert [int(x) for x in batches[:, 1]] == counts
    whole = iref.expected(s)   # the un-culled frame: the same picture, other owners' numbers
    np.testing.assert_array_equal(got["depth"].view(np.uint32), whole["depth"].view(np.uint32))
    np.testing.assert_array_equal(got["covered"], whole["covered"])
    assert ref.same_bits_or_class(got["planes"], whole["planes"]).all()


def test_the_chain_behind_a_wall_with_the_pyramid_of_its_depth(ctx):
    build, counts = cases.CHAINS["chain_occlusion"]
    c = build()
    s = c["scene"]
    w, h, levels = c["hiz"]
    up = Uploaded(ctx, s)
    # the wall's depth: the first draw alone, on the device (bit for bit the restatement's) -> sailor_hip_hiz_build
    wall = dict(iref.survivors(s), draws=iref.survivors(s)["draws"][:1])
    wall_want = iref.renderer(wall)(wall)
    sp = SurfacePass(ctx, s["W"], s["H"], max_draws=len(s["draws"]))
    sp.begin()
    sp.draw_indirect(up.frame, instances=up.instances, command=up.commands, command_index=0, capacity=1, num_instance_records=s["records"], **up.draws[0])
    depth = up.resolve(sp)["depth"]
    np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), wall_want["depth"].view(np.uint32))
    pyramid = hiz_build(ctx, depth, w, h, levels)
    want_pyramid = oracle.hiz_build(wall_want["depth"], w, h, levels)
    np.testing.assert_array_equal(pyramid.cpu().numpy().view(np.uint32), want_pyramid.view(np.uint32))
    mc = MeshCull(ctx, padded_records(s), c["batches"])
    out = chain_pass(c, up, mc, sp, hiz=(pyramid, w, h, levels))
    got = downloaded(sp, out)
    after, want_counts = cases.chain_after_cull(c, (want_pyramid, w, h, levels))
    assert want_counts == counts == [1, 0]
    assert_same(got, iref.expected(after), after, "the chain behind the wall")
    _, batches = mc.download()
    assert [int(x) for x in batches[:, 1]] == counts
    np.testing.assert_array_equal(got["depth"].view(np.uint32), wall_want["depth"].view(np.uint32))   # the frame is the wall's
    assert ref.same_bits_or_class(got["planes"], wall_want["planes"]).all() and got["covered"].all()


def test_the_chain_captured_once_and_replayed_over_two_sets_of_records(ctx):
    """cull + begin + indirect draws + resolve as a linear chain on a side stream; the records and the host's commands are copied into the SAME buffers at the
    head of the graph from staging tensors that change between the replays: each replay is its own records' frame, so the counts are read when the kernels run"""
    chains = [cases.CHAINS[n][0]() for n in ("chain_frustum", "chain_frustum_turned")]
    wants = []
    for c in chains:
        after, _ = cases.chain_after_cull(c)
        wants.append((after, iref.expected(after)))
    assert not np.array_equal(wants[0][1]["keys"], wants[1][1]["keys"])
    side = torch.cuda.Stream(device=ctx.device)
    c2 = HipContext(ctx.device, stream=side)
    try:
        c, s = chains[0], chains[0]["scene"]
        up = Uploaded(c2, s)
        mc = MeshCull(c2, padded_records(s), c["batches"])
        sp = SurfacePass(c2, s["W"], s["H"], max_draws=len(s["draws"]))
        staged_records, staged_commands = mc.instances.clone(), mc.batches.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            mc.instances.copy_(staged_records); mc.batches.copy_(staged_commands)   # what the host's UpdateBuffer does every frame
            out = chain_pass(c, up, mc, sp)
        for which in (0, 1, 0):
            staged_records.copy_(dev(c2, padded_records(chains[which]["scene"]).view(np.uint8)))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            after, want = wants[which]
            assert_same(downloaded(sp, out), want, after, f"replay over the records of chain {which}")
    finally:
        c2.close()
