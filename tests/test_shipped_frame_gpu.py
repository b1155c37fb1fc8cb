"""tests/golden/DefaultRenderer.renderer as shipped, entry by entry: three frames of it are captured between their entries (Runtime.capture_next_frame) and
every entry is judged by tests/frame_stages.py on the state the GPU itself held in front of it.

  * every resource an entry writes equals the stage's reference applied to the captured state before the entry, bit for bit (the bound of every stage that has
    a reference, and every entry has one -- except the radiance RenderScene composites (1e-4 relative, no absolute floor, no pixel left out), the Sky
    node's planes (1e-4 relative, equal classes, no texel left out) and the BRDF table (2e-6 absolute); the Environment node's bake and the Sky bake's two
    mip-generation frames run in frames that are not captured, see tests/frame_stages.py);
  * whether AO reaches `Main`: on 96 x 96 the Opaque RenderScene differs from its reference evaluated with ao = 1, on 128 x 96 it equals it (the documented
    simplification of the shipped g_AO extent, pinned as it is); on the warm frames the ambient term is non-zero;
  * every named resource an entry does not write is bit-identical before and after it -- for all 23 entries, and for the frame's transfer list;
  * no stage passes vacuously: the reference's output differs from the state before it, the Masked prepass discards some fragments and keeps some, some tile
    lists two lights or more;
  * four mutants of the shipped text (HBAO occlusionPower, Bloom threshold, MotionBlur data.samples, the two HBAO_Blur outputs swapped) are each caught at
    their own entry while the table keeps reading the shipped text;
  * a frame processed armed and the same frame processed unarmed leave the same bits in every named resource and the same launch log; arming while the
    stream is captured into a hipGraph is refused.

The scene is tests/shadow_prepass_cases.py's (ground strips and boxes under one directional EVSM light) with a checker-alpha quad under `Masked`, point and
spot lights, a few debug lines and one small ImGui list.  Frames: 128 x 96 cold; 128 x 96 warm -- the first frame after the Sky node's cube bake has reached
Environment (the bake's length is read from the node), with the camera moved; 96 x 96 warm, the square case."""
import copy
import functools

import numpy as np
import pytest
import torch

import frame_stages as fs
import masked_cases
import shadow_prepass_cases as sc
import surface_cases as cases
import ui_cases
from hbao_cases import noise_texels
from sailor_amd import _lib, host, synth
from sailor_amd.forward_plus import upload_textures
from sailor_amd.runtime_binding import Runtime

pytestmark = pytest.mark.gpu
f32 = np.float32
EVSM = 2
POINT, SPOT = 1, 2
SIZES = (64, 128, 256, 64)
DT = 1.0 / 60.0
BATCH_ALPHA_CUTOUT, BATCH_DOUBLE_SIDED = 1, 2
MIN_LIVE_SHARE = 0.01    # of the words a reference determines, the share that must differ from the state before the entry
MAX_BAKE_FRAMES = 32
MOVED = (3.0, 152.0, -5.0)
BAKED = {"g_envCubemap", "g_irradianceCubemap"}   # created by the Environment node's bake, in the frame in which the Sky node's cube bake ends


def camera(width, height, position=(0.0, 150.0, 0.0)):
    cam = synth.make_camera(width, height, z_far=sc.Z_FAR)
    cam.world = host.transform_matrix([*position, 1.0], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0])
    cam.frame = host.fill_frame_data(cam.world, cam.fov, cam.z_near, cam.z_far, cam.width, cam.height)
    return cam


@functools.lru_cache(maxsize=None)
def scene_arrays():
    """shadow_prepass_cases' layout plus one quad with a 4 x 4 alpha checker in front of the camera, its batch tagged Masked (ALPHA_CUTOUT, double-sided)"""
    L = sc.layout(False)
    qv, qt = cases.quad(-1, -1, 1, 1, z=0.0, uv=((0, 0), (3, 0), (3, 3), (0, 3)))
    first_vertex, first_index, first_instance = len(L.vertices), len(L.indices), L.num_instances
    model = host.transform_matrix([0.0, 150.0, -30.0, 1.0], [0.0, 0.0, 0.0, 1.0], [10.0, 8.0, 1.0, 1.0])
    # (through bytes: concatenating the records themselves would repack the dtype without its padding)
    inst = np.concatenate([a.view(np.uint8).reshape(-1, 96) for a in (L.instances, cases.instances([model], [2]))]).reshape(-1).view(host.INSTANCE_DTYPE).copy()
    assert len(inst) == first_instance + 1
    inst["sphereBounds"][:] = (0.0, 0.0, 0.0, np.sqrt(3.0))   # model space: the unit cube's, and more than either quad's
    box = f32([-10.0, 142.0, -30.0, 10.0, 158.0, -30.0])
    box[:3], box[3:] = np.nextafter(box[:3], f32(-np.inf)), np.nextafter(box[3:], f32(np.inf))
    return dict(vertices=np.concatenate([L.vertices, np.asarray(qv, f32)]), indices=np.concatenate([L.indices, np.asarray(qt, np.uint32).reshape(-1)]).astype(np.uint32),
                instances=inst, materials=np.concatenate([L.materials, cases.material(albedo=(0.8, 0.9, 0.3, 1), metallic=0.1, roughness=0.7, samplers=(3, 2, 1, 2))]),
                textures=L.textures + [masked_cases.checker(4)], srgb=L.srgb + [True],
                batches=np.concatenate([L.batches, np.uint32([[6, 1, first_index, first_vertex, first_instance]])]), tags=["Opaque", "Opaque", "Masked"],
                flags=[0, 0, BATCH_ALPHA_CUTOUT | BATCH_DOUBLE_SIDED], world_aabb=np.concatenate([L.world_aabb, box[None]]),
                last_changed_frames=np.concatenate([L.last_changed_frames, np.zeros(1, np.uint64)]))


def cube_chain_bytes(size, levels, texel=16):
    return sum(6 * max(1, size >> l) ** 2 for l in range(levels)) * texel


class HostView:
    """one slot of a captured frame as the references see it: name -> flat uint32 array, downloaded when asked for"""

    def __init__(self, slot):
        self.slot, self.cache = slot, {}

    def __contains__(self, name):
        return name in self.slot

    def __getitem__(self, name):
        if name not in self.cache:
            self.cache[name] = self.slot[name].cpu().numpy().view(np.uint32)
        return self.cache[name]


class Shipped:
    """one runtime over the scene at a viewport, fed the way tests/test_default_renderer_gpu.py feeds it; `text` is what the RUNTIME loads"""

    def __init__(self, ctx, width, height, text=None):
        self.W, self.H, self.ctx = width, height, ctx
        self.targets, self.table = fs.stages()   # always the shipped text
        dev = ctx.device
        s = scene_arrays()
        self.keep = [torch.from_numpy(s["vertices"]).to(dev), torch.from_numpy(s["indices"].view(np.int32)).to(dev), torch.from_numpy(s["instances"].view(np.uint8).copy()).to(dev),
                     torch.from_numpy(s["materials"].view(np.uint8).copy()).to(dev), torch.from_numpy(s["world_aabb"]).to(dev)]
        textures, num_textures, keep = upload_textures(ctx, s["textures"], s["srgb"])
        self.keep += [textures, keep]
        self.depth_buffer = torch.full((height, width), 0.75, dtype=torch.float32, device=dev)
        self.back = torch.full((height, width, 4), -3.0, dtype=torch.float32, device=dev)
        self.noise_host = np.ascontiguousarray(noise_texels(), f32)
        self.dirt_host = np.random.default_rng(5).uniform(0, 1, (32, 32, 4)).astype(f32)
        self.noise, self.dirt = torch.from_numpy(self.noise_host).to(dev), torch.from_numpy(self.dirt_host).to(dev)
        self.cam = camera(width, height)
        self.rt = rt = Runtime(0, torch.cuda.current_stream().cuda_stream)
        try:
            rt.set_camera(self.cam)
            for node in ("Clear", "ShadowPrepass", "Bloom"):
                rt.enable_node(node)
            for shader in ("Shaders/MotionBlur.shader", "Shaders/Debug.shader"):
                rt.enable_shader(shader)
            created, skipped, _ = rt.load_renderer(fs.shipped_text() if text is None else text)
            assert (created, skipped) == (len(self.table), 0), (created, skipped)
            rt.set_render_target("DepthBuffer", self.depth_buffer)
            rt.set_color_target("BackBuffer", self.back)
            assert rt.set_sampler("g_noiseSampler", self.noise, self.noise.shape[1], self.noise.shape[0]) == 0
            assert rt.set_sampler("g_lensDirtSampler", self.dirt, 32, 32) == 0
            sun = rt.add_light(0, EVSM, sc.LIGHT_POSITION, [0.0, -1.0, 0.0], [3.0, 3.0, 3.0], [100.0, 100.0, 100.0])
            rt.set_light_rotation(sun, sc.LIGHT_ROTATION)
            for position, colour in (((0.0, 72.0, -60.0), (40.0, 10.0, 10.0)), ((12.0, 72.0, -70.0), (10.0, 40.0, 10.0)), ((-45.0, 75.0, -150.0), (10.0, 10.0, 40.0)),
                                     ((60.0, 80.0, -220.0), (30.0, 30.0, 5.0))):
                rt.add_light(POINT, 0, position, [0.0, 0.0, -1.0], colour, [40.0, 40.0, 40.0])
            rt.add_light(SPOT, 0, (20.0, 120.0, -100.0), [0.0, -1.0, 0.0], (50.0, 50.0, 50.0), [80.0, 80.0, 80.0], cut_off_degrees=(25.0, 40.0))
            rt.tick_lights()
            rt.set_scene(self.keep[0], self.keep[1], self.keep[2], self.keep[3], textures, num_textures, s["batches"])
            rt.set_scene_tags(s["tags"], s["flags"])
            rt.set_caster_data(self.keep[4], s["last_changed_frames"], resolutions=SIZES, trace="flat")
            rt.debug_draw_line([-20.0, 130.0, -60.0], [25.0, 165.0, -90.0], (1.0, 0.5, 0.0, 1.0), duration=1000.0)
            rt.debug_draw_aabb([-30.0, 100.0, -120.0], [30.0, 140.0, -80.0], (1.0, 1.0, 0.0, 1.0), duration=1000.0)
            rt.debug_draw_arrow([-40.0, 70.0, -50.0], [35.0, 150.0, -140.0], (0.2, 0.9, 0.3, 1.0), duration=1000.0)
            self.ui = fs.ui_draw_data(width, height)
            assert rt.set_ui_draw_data(self.ui, font=ui_cases.ATLAS) > 0
        except BaseException:
            rt.close()
            raise
        # a defined state in front of the cold frame: every render target the file declares holds the sentinel the caller's BackBuffer holds, so that the
        # liveness share of the first frame does not rest on what the allocations happened to hold
        for name in self.targets:
            ptr, w, h, levels = rt.render_target(name)
            words = fs.chain_words(w, h, fs.target_dims(self.targets, width, height)[name][2], levels)
            _lib.check(ctx._lib.sailor_hip_buffer_fill_u32(ctx.handle, ptr, 0, int(f32(-3.0).view(np.uint32)), words), "sailor_hip_buffer_fill_u32", ctx.handle)
        ctx.synchronize()
        self.frames, self.time, self.previous = 0, 0.0, _lib.UboFrameData()
        self.names = fs.capture_names(self.targets, self.table)
        self.dims = fs.target_dims(self.targets, width, height)
        self.dims["BackBuffer"], self.dims["DepthBuffer"] = (width, height, 4, 1), (width, height, 1, 1)
        tx, ty = host.num_tiles(width, height)
        caps = {name: fs.chain_words(*d) * 4 for name, d in self.dims.items()}
        caps.update(lightsGrid=4 * (tx * ty * 2 + 1), culledLights=4 * (tx * ty * fs.LIGHTS_PER_TILE + 1), light=rt.buffer("light")[1], lightsMatrices=256, eyeAdaptation=8192,
                    g_irradianceCubemap=cube_chain_bytes(32, 1), g_envCubemap=cube_chain_bytes(256, 8), g_skyCubemap=cube_chain_bytes(256, 8), g_brdfSampler=256 * 256 * 8)
        caps.update({f"csm{k}": SIZES[k] * SIZES[k] * 16 for k in range(4)})
        caps.update({name: 64 * 20 for name in self.names if name.startswith("indirect")})
        self.capacities = {name: caps[name] for name in self.names}

    def close(self):
        self.rt.close()

    def step(self, cam=None, capture=False, status=0):
        """one frame -> (slots or None, FrameData, the frame's launch count and the last launches' names)"""
        rt = self.rt
        if cam is not None:
            self.cam = cam
        rt.set_camera(self.cam)
        rt.set_time(DT, self.time)
        assert rt.debug_tick(DT) > 0
        storage = None
        if capture:
            storage = torch.zeros((len(self.table) + 2) * sum(self.capacities.values()), dtype=torch.uint8, device=self.back.device)
            assert rt.capture_next_frame(self.capacities, storage) == len(self.table) + 2
        launched, _ = rt.launch_log(0)
        sky_state = rt.sky_state()
        assert rt.process_frame() == status   # (-1: the driver refused a command with the invalid-argument status)
        rt.wait_idle()
        torch.cuda.synchronize()
        after, names = rt.launch_log(16)
        c = self.cam
        frame = host.fill_frame_data(c.world, c.fov, c.z_near, c.z_far, self.W, self.H, self.time, DT, aspect=c.aspect)
        hist, lum = rt.eye_adaptation_state()
        fd = fs.FrameData(self.W, self.H, frame, self.previous, DT, self.frames == 0, self.dims, num_lights=rt.total_num_lights(), noise=self.noise_host, dirt=self.dirt_host,
                          eye_luminance_word=(lum - hist) // 4, debug_vertices=rt.debug_vertices(), ui=(host.ui_flatten(self.ui), ui_cases.ATLAS), camera=copy.copy(c),
                          light_view=sc.light_view(), shadow_cascades=tuple(p["cascade"] for p in rt.shadow_passes()), scene=scene_arrays(), sky_state=sky_state, ctx=self.ctx, shadow_passes=tuple(rt.shadow_passes(len(scene_arrays()["instances"]))),
                          sky_light=tuple(host.sky_params().lightDirection))
        self.previous, self.frames, self.time = frame, self.frames + 1, self.time + DT
        slots = rt.captured_frame() if capture else None
        if slots:
            fd.words = {name: t.numel() // 4 for name, t in slots[-1].items()}
        self.storage = storage   # the slots are views of it
        return slots, fd, (after - launched, names)

    def bake(self):
        """process frames until the Sky node's time-sliced cube bake has finished -- in that frame it marks Environment dirty, which bakes in the same frame --
        and return how many frames that took: the node's own count, nothing here knows it"""
        n = 0
        while self.rt.sky_state()[1]:
            assert n < MAX_BAKE_FRAMES, "the Sky node never finishes its bake"
            self.step()
            n += 1
        return n


def same_words(a, b):
    return a.numel() == b.numel() and torch.equal(a.view(torch.int32), b.view(torch.int32))


def untouched(names, writes, before, after, what):
    """every named resource outside `writes` holds the same bits before and after (or is absent both times) -> failures"""
    out = []
    for name in names:
        if name in writes:
            continue
        if (name in before) != (name in after):
            out.append(f"{what}: {name} {'appeared' if name in after else 'disappeared'} and is not among its writes")
        elif name in before and not same_words(before[name], after[name]):
            differ = int((before[name].view(torch.int32) != after[name].view(torch.int32)).sum()) if before[name].numel() == after[name].numel() else -1
            out.append(f"{what}: wrote {name} ({differ} words differ), which is not among its writes")
    return out


def judge(run, slots, fd, upto=None):
    """-> rows, one per entry (and one for the transfer list): dict(index, label, checked, bound, worst, left_out, live, failures)"""
    fd.frame_start = HostView(slots[0])
    rows = [dict(index=-1, label="(transfer list)", checked=(), bound="", worst="", left_out=0.0, live=None,
                 failures=untouched(run.names, fs.transfer_writes(run.table), slots[0], slots[1], "the transfer list"))]
    for s in run.table:
        if upto is not None and s.index > upto:
            break
        before, after = slots[1 + s.index], slots[2 + s.index]
        row = dict(index=s.index, label=s.label, checked=(), bound="", worst="", left_out=0.0, live=None, failures=untouched(run.names, s.writes, before, after, s.label))
        if s.reference is not None:
            state, got_state = HostView(before), HostView(after)
            want = s.reference(state, fd)
            assert set(want) <= set(s.writes), (s.label, sorted(want))
            for name in s.writes:   # a write the reference says nothing about is a resource that does not exist yet, or one listed as still to be restated
                if name not in want and name not in fs.PARTLY_PENDING.get(s.index, ()) and name in after:
                    row["failures"].append(f"{s.label}: the reference says nothing about {name}")
            determined = wrong = total = live_words = 0
            differing = 0.0
            for name, e in want.items():
                if name not in after:
                    row["failures"].append(f"{s.label}: {name} does not exist after the entry")
                    continue
                got = got_state[name]
                mask = np.ones(e.words.size, bool) if e.mask is None else e.mask
                ok = fs.same_bits_or_class(got, e.words)
                if e.rtol_mask is not None:   # relative with no absolute floor (or the stage's absolute bound), a non-finite word by its class, no word left out
                    g, w = got.view(f32).astype(np.float64), e.words.astype(np.float64)
                    with np.errstate(all="ignore"):
                        err = np.abs(g - w)
                        close = err < e.atol if e.atol is not None else err <= fs.RADIANCE_RTOL * np.abs(w)
                        ok = np.where(e.rtol_mask, np.where(np.isfinite(w), close, ok), ok)
                        rel = np.where(e.rtol_mask & np.isfinite(w) & (w != 0), err if e.atol is not None else err / np.abs(w), 0.0)
                    row["abs" if e.atol is not None else "rel"] = max(row.get("abs" if e.atol is not None else "rel", 0.0), float(np.nanmax(rel)))
                ok = ok | ~mask
                if not ok.all():
                    first = int(np.argmin(ok))
                    row["failures"].append(f"{s.label}: {int((~ok).sum())} of {int(mask.sum())} words of {name} differ from the reference, first at word {first}: "
                                           f"{got.view(e.words.dtype)[first]!r} != {e.words[first]!r}")
                wrong += int((~ok).sum())
                determined += int(mask.sum()); total += mask.size
                if not e.unchanged:   # liveness: of the resources the entry has work on, the one whose determined words differ most from the state before
                    live_words += int(mask.sum())   # (per resource, not pooled: a map or a cube the frame itself allocates holds whatever the allocation held)
                    share = int(((fs.prior(fd, state, name) != e.words.view(np.uint32)) & mask).sum()) / max(int(mask.sum()), 1)
                    differing = max(differing, share)
            within = "; ".join([f"{k} {row[k]:.2e}" for k in ("rel", "abs") if k in row] + [fs.BITS if not any(k in row for k in ("rel", "abs")) else "bits"])
            # live None: the entry has nothing to do in this frame (every write expected unchanged)
            row.update(checked=tuple(want), bound=s.bound, worst=within if wrong == 0 else f"{wrong} words differ", left_out=1.0 - determined / max(total, 1),
                       live=differing if live_words else None, idle=live_words == 0)
        else:
            row.update(bound="none", worst=s.note)
        rows.append(row)
    return rows


def show(title, rows):
    print(f"\n{title}")
    print(f"{'entry':>5}  {'stage':<34} {'checked':<28} {'bound':<12} {'worst':<22} {'left out':>9} {'live':>7}")
    for r in rows:
        live = "" if r["live"] is None else f"{100 * r['live']:.1f}%"
        print(f"{r['index']:>5}  {r['label']:<34} {','.join(r['checked']):<28} {r['bound']:<12} {r['worst'][:60]:<22} {100 * r['left_out']:>8.2f}% {live:>7}")
    for r in rows:
        for f in r["failures"]:
            print("   FAIL", f)


def failures_of(rows):
    return [f for r in rows for f in r["failures"]]


# ---- the three frames -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames(ctx):
    """name -> (run's table and names, slots, FrameData, rows, extra): judged once, shared by the tests below and left unchanged"""
    out = {}
    for width, height in ((128, 96), (96, 96)):
        run = Shipped(ctx, width, height)
        try:
            if (width, height) == (128, 96):
                slots, fd, _ = run.step(capture=True)
                out["cold 128x96"] = dict(run=run, fd=fd, rows=judge(run, slots, fd), facts=facts(run, slots, fd), pins=pins_of(run, slots, fd))
            else:
                run.step()
            baked = run.bake()
            slots, fd, _ = run.step(cam=camera(width, height, MOVED), capture=True)
            out[f"warm {width}x{height}"] = dict(run=run, fd=fd, rows=judge(run, slots, fd), facts=facts(run, slots, fd), baked=baked, pins=pins_of(run, slots, fd))
            del slots
            run.storage = None
        finally:
            run.close()
    return out


def pins_of(run, slots, fd):
    """the Opaque RenderScene's Main against its reference evaluated with ao = 1 and without the ambient term -> counts of words"""
    import dataclasses
    s = next(s for s in run.table if s.label == "RenderScene Opaque")
    before, got = HostView(slots[1 + s.index]), HostView(slots[2 + s.index])["Main"].view(f32).astype(np.float64)
    out = {}
    for key, changes in (("ao_one_wrong", dict(force_ao_one=True)), ("no_ambient_wrong", dict(force_no_ambient=True))):
        e = s.reference(before, dataclasses.replace(fd, **changes))["Main"]
        w = e.words.astype(np.float64)
        out[key] = int((e.rtol_mask & ~(np.abs(got - w) <= fs.RADIANCE_RTOL * np.abs(w))).sum())
        out["covered"] = int(e.rtol_mask.sum())
    out["ambient_share"] = out.pop("no_ambient_wrong") / max(out["covered"], 1)
    return out


def facts(run, slots, fd):
    """what the liveness assertions need of a captured frame, taken while its storage is alive"""
    by_label = {s.label: s for s in run.table}
    masked, cull = by_label["DepthPrepass Masked"], by_label["LightCulling"]
    before, after = (HostView(slots[k + masked.index])["DepthBuffer"].view(f32).reshape(fd.height, fd.width) for k in (1, 2))
    kept = before != after
    ys, xs = np.nonzero(kept)
    holes = 0 if not kept.any() else int((~kept[ys.min():ys.max() + 1, xs.min():xs.max() + 1]).sum())
    tx, ty = host.num_tiles(fd.width, fd.height)
    grid = HostView(slots[2 + cull.index])["lightsGrid"][:tx * ty * 2].reshape(-1, 2)
    present = [sorted(slot) for slot in (slots[0], slots[-1])]
    return dict(kept=int(kept.sum()), holes=holes, lights_per_tile=(int(grid[:, 1].min()), int(grid[:, 1].max())), present=present)


@pytest.mark.parametrize("name", ["cold 128x96", "warm 128x96", "warm 96x96"])
def test_every_entry_of_the_shipped_frame(frames, name):
    f = frames[name]
    show(name, f["rows"])
    print("facts:", {k: v for k, v in f["facts"].items() if k != "present"}, "bake frames:", f.get("baked"))
    assert failures_of(f["rows"]) == []
    assert fs.PENDING == () and all(r["checked"] for r in f["rows"][1:])   # every entry has a reference
    idle = [r["label"] for r in f["rows"] if r.get("idle")]
    assert idle == ([] if name.startswith("cold") else ["Environment"]), idle   # the Environment node is not dirty on a warm frame: it must leave its samplers alone
    referenced = [r for r in f["rows"] if r["live"] is not None]
    assert len(referenced) == len(f["run"].table) - len(idle)
    for r in referenced:   # no stage passes vacuously, on any captured frame (the cold frame starts from sentinel-filled targets)
        assert r["live"] >= MIN_LIVE_SHARE, (name, r["label"], r["live"])
    # whether AO reaches Main: the Opaque RenderScene against the same reference evaluated with ao = 1.  The shipped g_AO is ViewportWidth squared and the driver
    # takes it only at the frame's extent ("HBAO", a kept simplification): on 96 x 96 the frame must NOT be the ao = 1 frame, on 128 x 96 it is
    pins = f["pins"]
    print("pins:", pins)
    if name.startswith("warm"):
        assert pins["ambient_share"] > 0.05, pins               # the ambient term is non-zero: without the IBL samplers the reference is another frame
        if name.endswith("96x96"):
            assert pins["ao_one_wrong"] > 0.05 * pins["covered"], pins   # AO reaches Main
        else:
            assert pins["ao_one_wrong"] == 0, pins                       # ao = 1: the documented simplification, pinned as it is
    else:
        assert pins["ambient_share"] == 0 and pins["ao_one_wrong"] == 0, pins   # no cubes yet: no ambient term, with or without AO
    assert f["facts"]["kept"] > 50 and f["facts"]["holes"] > 50, f["facts"]             # the Masked prepass keeps some fragments of the checker and discards some
    assert f["facts"]["lights_per_tile"][1] >= 2, f["facts"]                            # some tile lists two lights or more
    if name.startswith("cold"):   # a cube does not exist before the frame that creates it -- the baked ones not before the Sky node's bake has ended: absent, not an error
        assert not {"g_skyCubemap", "g_envCubemap", "g_irradianceCubemap", "g_brdfSampler"} & set(f["facts"]["present"][0])
        assert set(f["run"].names) - set(f["facts"]["present"][1]) == BAKED
    else:   # at a warm frame's end every named resource exists
        assert set(f["facts"]["present"][1]) == set(f["run"].names), set(f["run"].names) - set(f["facts"]["present"][1])
        assert 1 <= f["baked"] <= MAX_BAKE_FRAMES


# ---- the mutants ------------------------------------------------------------------------------------------------------------------------------------------
def swap_blur_outputs(text):
    assert text.count("  - color: TemporaryR8\n") == 1 and text.count("  - color: g_AO\n") == 1
    return text.replace("  - color: TemporaryR8\n", "  - color: @\n").replace("  - color: g_AO\n", "  - color: TemporaryR8\n").replace("  - color: @\n", "  - color: g_AO\n")


def replace_once(old, new):
    def mutate(text):
        assert text.count(old) == 1, old
        return text.replace(old, new)
    return mutate


MUTANTS = {
    "HBAO occlusionPower": (replace_once("  - data.occlusionPower: 1.5\n", "  - data.occlusionPower: 2.5\n"), ("HBAO",)),
    "Bloom threshold": (replace_once("  - threshold: [3.0, 0, 0, 0]\n", "  - threshold: [0.5, 0, 0, 0]\n"), ("Bloom",)),
    "MotionBlur data.samples": (replace_once("  - data.samples: 10\n", "  - data.samples: 4\n"), ("MotionBlur",)),
    "HBAO_Blur outputs swapped": (swap_blur_outputs, ("HBAO_Blur VERTICAL", "HBAO_Blur HORIZONTAL")),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_shipped_text_is_caught_at_its_own_entry(ctx, name):
    """the runtime loads the shipped text with one value changed, the table keeps reading the shipped text: the changed entry's check -- and no earlier one --
    reports a mismatch (the swapped outputs change two entries: both report)"""
    mutate, labels = MUTANTS[name]
    run = Shipped(ctx, 128, 96, text=mutate(fs.shipped_text()))
    try:
        last = max(s.index for s in run.table if s.label in labels)
        # (swapped, the horizontal blur would read and write TemporaryR8 in one launch: the driver refuses that draw with the invalid-argument status, which
        # is the frame's; every other mutant is a clean frame)
        slots, fd, _ = run.step(capture=True, status=-1 if name == "HBAO_Blur outputs swapped" else 0)
        rows = judge(run, slots, fd, upto=last)
    finally:
        run.close()
    show(f"mutant: {name}", rows)
    failing = {r["label"] for r in rows if r["failures"]}
    assert failing == set(labels), (name, failing, failures_of(rows)[:4])


# ---- the facility itself ----------------------------------------------------------------------------------------------------------------------------------
def test_an_armed_frame_and_an_unarmed_frame_are_the_same_frame(ctx):
    """two fresh runtimes process frame 1, one armed and one not; both then capture frame 2, whose slot 0 is the state frame 1 left: the same bits in every
    named resource, the same number of launches in frame 1 and the same last launches (the capture's copies are no launches)"""
    ends, logs = [], []
    for armed in (True, False):
        run = Shipped(ctx, 128, 96)
        try:
            _, _, log = run.step(capture=armed)
            slots, _, _ = run.step(capture=True)
            ends.append({name: t.clone() for name, t in slots[0].items()})
            logs.append(log)
        finally:
            run.close()
    assert logs[0] == logs[1], logs
    assert sorted(ends[0]) == sorted(ends[1]) and set(ends[0]) == set(run.names) - BAKED
    different = [name for name in ends[0] if not same_words(ends[0][name], ends[1][name])]
    assert different == [], different


def test_arming_is_refused_while_the_stream_is_captured_into_a_graph(ctx):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rt = Runtime(0, side.cuda_stream)
    try:
        storage = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.device)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.SailorHipError):
                rt.capture_next_frame({"BackBuffer": 1024}, storage)
            storage.add_(1)   # (the graph holds something)
        del graph
        assert rt.capture_next_frame({"BackBuffer": 1024}, storage) == 2   # an empty graph: the two slots around no entry
        with pytest.raises(_lib.SailorHipError):
            rt.capture_next_frame({"BackBuffer": 1 << 20}, storage)         # too little storage for the slots
    finally:
        rt.close()
