"""tests/golden/DefaultRenderer.renderer as a table of stages: one per `frame:` entry, in file order, parsed from the shipped text AS TEXT.

A stage says which named resources its entry may read, which it may write, and -- where this table has one -- a reference function

    reference(before: dict name -> flat uint32 array, fd: FrameData) -> dict name -> Expected

over the state the GPU itself held in front of the entry (Runtime.capture_next_frame), for everything the entry writes.  Every reference calls the
restatement the per-node runtime test of that kernel already uses and is held to the bound that test uses: bit for bit (`same_bits_or_class`: finite words by
their bits, non-finite ones by class), and for the radiance RenderScene composites onto the covered pixels of `Main` 1e-4 relative with no absolute floor
(BASELINE.json, test_shade_gpu.RTOL) with no pixel left out.  No stage of this table has a tolerance of its own.  A reference may leave words of a resource
undetermined (Expected.mask): the word behind lightsGrid's last record, the culledLights slots behind the listed indices, the words of the EyeAdaptation
state that are neither a count nor the adapted luminance.  Nobody reads those; their share is printed and not capped.  Parameters come from the shipped text through `Params`, which
records the keys a reference asked for: tests/test_frame_stages_cpu.py fails for a parameter line no reference reads.

Resources are flat uint32 arrays (the bytes as captured); `FrameData.dims` gives their geometry.  Besides the render targets of the file the names are
BackBuffer and DepthBuffer (the caller's per-frame targets), lightsGrid / culledLights / light / lightsMatrices, csm0 .. csm3, the three IBL samplers,
g_skyCubemap, eyeAdaptation (256 histogram counts, then the node's state with the adapted luminance at word FrameData.eye_luminance_word) and
indirect<i> (the indirect commands of entry i).

Other bounds in use: the Sky target and the cube face the Sky node bakes in a frame against sky_ref.Ref32 at 1e-4 relative with equal classes and no texel
left out (tests/test_sky_runtime_gpu.py); the BRDF table against the C oracle at 2e-6 absolute (tests/test_ambient_gpu.py).  The cascade maps are held, bit for
bit, to the C-ABI sequence of tests/test_shadow_prepass_runtime_gpu.py (a), which needs the device (FrameData.ctx).

PENDING and PARTLY_PENDING are empty: every entry has a reference for every write.  What the captured frames do NOT hold, because no captured frame runs it:
the Environment node's bake (it runs once, in the frame in which the Sky node's bake ends; its float64 restatement at the shipped sizes takes minutes and the
file has no knob for the sizes) and the two mip-generation frames of the Sky node's bake.  On the warm frames the Environment stage is held to leaving its
samplers alone, and the baked cubes are what RenderScene's reference reads."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

f32 = np.float32
ROOT = Path(__file__).resolve().parents[1]
SHIPPED = ROOT / "tests" / "golden" / "DefaultRenderer.renderer"
OUTPUT_ROLES = ("color", "target", "dst", "bloom")
BITS = "bit for bit"
RADIANCE_RTOL = 1e-4   # BASELINE.json, tests/test_shade_gpu.py RTOL: relative, no absolute floor
SKY_REL = RADIANCE_RTOL   # tests/test_sky_runtime_gpu.py REL: the Sky target against sky_ref.Ref32, classes equal, no texel left out
BRDF_ATOL = 2e-6         # tests/test_ambient_gpu.py test_brdf_lut_matches_the_oracle: 1 024-term sums, libm against device trigonometry
SKY_CUBE_SIZE, SKY_CUBE_LEVELS = 256, 8   # SkyNode.h:13 EnvCubemapSize and the chain the node creates
RADIANCE = "1e-4 rel; bits"   # radiance of the covered pixels at RADIANCE_RTOL, every other word of the target bit for bit
BOUNDS = {"RenderScene": RADIANCE, "Sky": "1e-4 rel, classes", "Environment": "2e-6 abs; bits"}
PER_FRAME_TARGETS = ("BackBuffer", "DepthBuffer")   # named by the entries, declared by nobody: the caller's
LIST_BUFFERS = ("lightsGrid", "culledLights")
CASCADES = ("csm0", "csm1", "csm2", "csm3")
IBL_SAMPLERS = ("g_irradianceCubemap", "g_envCubemap", "g_brdfSampler")
LIGHTS_PER_TILE = 128


def shipped_text() -> str:
    return SHIPPED.read_text()


# ---- the text ------------------------------------------------------------------------------------------------------------------------------------------
def _value(raw: str) -> str:
    """the scalar behind `key:`: a `#` at its start or after a blank begins a comment, `~` is null, quotes go"""
    raw = raw.strip()
    if raw.startswith("#"):
        return ""
    raw = re.split(r"\s+#", raw, maxsplit=1)[0].strip()
    return "" if raw == "~" else raw.strip("'\"")


class Params:
    """the parameter lines of one entry; every look-up is recorded in `used` as (section, key)"""

    def __init__(self, lines):
        self.lines = dict(lines)   # (section, key) -> text
        self.used = set()

    def _get(self, section, key):
        self.used.add((section, key))
        return self.lines[(section, key)]

    def has(self, section, key):
        return (section, key) in self.lines

    def string(self, key):
        return self._get("string", key)

    def flag(self, key):
        """a `string:` line that holds a boolean; absent = false"""
        return self.has("string", key) and self._get("string", key).lower() == "true"

    def float(self, key):
        return float(self._get("float", key))

    def vec4(self, key):
        body = self._get("vec4", key).strip()
        assert body.startswith("[") and body.endswith("]"), body
        v = [float(x) for x in body[1:-1].split(",")]
        assert len(v) == 4, body
        return v

    def target(self, role):
        return self._get("renderTargets", role)

    def unused(self):
        return sorted(set(self.lines) - self.used)


@dataclass
class Entry:
    index: int
    name: str
    params: Params
    roles: dict   # role -> resource name, in file order


def parse(text: str):
    """-> (targets: name -> dict(width, height as the file's expressions, channels, mips (bool), max_mip), entries)"""
    head, frame = text[:text.index("\nframe:")], text[text.index("\nframe:") + 1:]
    targets = {}
    section = head[head.index("\nrenderTargets:"):]
    for block in re.split(r"^- name: ", section, flags=re.M)[1:]:
        lines = [l for l in block.splitlines() if l.strip() and not l.strip().startswith("#")]
        fields = {k.strip(): _value(v) for k, v in (l.split(":", 1) for l in lines[1:])}
        targets[_value(lines[0])] = dict(width=fields["width"], height=fields["height"], channels=4 if re.match(r"R\d+G\d+B\d+A\d+_", fields["format"]) else 1,
                                        mips=fields.get("bGenerateMips", "false") == "true", max_mip=int(fields.get("maxMipLevel", 10000)))
    entries = []
    for block in re.split(r"^- name: ", frame, flags=re.M)[1:]:
        lines, roles, heading = {}, {}, None
        rows = block.splitlines()
        for row in rows[1:]:
            s = row.strip()
            if not s or s.startswith("#"):
                continue
            if s.startswith("- "):
                key, raw = s[2:].split(":", 1)
                assert heading, row
                lines[(heading, key.strip())] = _value(raw)
                if heading == "renderTargets":
                    roles[key.strip()] = _value(raw)
            else:
                heading = s.split(":", 1)[0].strip()
        entries.append(Entry(len(entries), _value(rows[0]), Params(lines), roles))
    return targets, entries


def extent(expression: str, width: int, height: int) -> int:
    """FrameGraphParser.cpp:66-77: `ViewportWidth[/k]`, `ViewportHeight[/k]` or a number"""
    m = re.fullmatch(r"(ViewportWidth|ViewportHeight)(?:/(\d+))?", expression)
    if not m:
        return int(expression)
    base = width if m.group(1) == "ViewportWidth" else height
    return max(1, int(f32(base) * (f32(1.0) / f32(int(m.group(2))) if m.group(2) else f32(1.0))))


def target_dims(targets, width, height):
    """name -> (w, h, channels, levels) of the declared render targets at a viewport (FrameGraphParser.cpp:205-208)"""
    out = {}
    for name, t in targets.items():
        w, h = extent(t["width"], width, height), extent(t["height"], width, height)
        levels = min(t["max_mip"], int(np.floor(np.log2(f32(max(w, h))))) + 1 if t["mips"] else 1)
        out[name] = (w, h, t["channels"], levels)
    return out


def chain_extents(w, h, levels):
    return [(max(1, w >> l), max(1, h >> l)) for l in range(levels)]


def chain_words(w, h, channels, levels):
    return sum(a * b for a, b in chain_extents(w, h, levels)) * channels


# ---- what a reference sees ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class FrameData:
    """what the harness fed the frame besides the captured state"""
    width: int
    height: int
    frame: object           # UboFrameData of this frame (sailor_host_fill_frame_data over the camera, the viewport and the frame's times)
    previous: object        # UboFrameData the graph uploaded as previousFrameData: all zeros on a graph's first frame
    delta_time: float
    first_frame: bool       # the graph's first frame: the nodes create and initialise their state inside it
    dims: dict              # name -> (w, h, channels, levels)
    num_lights: int = 0
    noise: np.ndarray | None = None   # g_noiseSampler's texels, float32 [h, w, 4]
    dirt: np.ndarray | None = None    # g_lensDirtSampler's texels
    eye_luminance_word: int = 256
    debug_vertices: np.ndarray | None = None   # the DebugContext's line list (VertexP3C4 records) this frame draws
    ui: tuple | None = None                    # (host.ui_flatten of the frame's draw data, the font atlas)
    camera: object = None                      # the scene view's camera
    light_view: np.ndarray | None = None       # the directional light's view matrix
    shadow_cascades: tuple = ()                # the cascades LightingECS planned a pass for in this frame
    words: dict = field(default_factory=dict)  # name -> length in words of the resources a node creates inside the frame (absent in front of it)
    scene: dict | None = None                  # the scene's host arrays: vertices, indices, instances, materials, textures, srgb, batches, tags, flags
    force_ao_one: bool = False                 # evaluate RenderScene's reference with ao = 1 whatever g_AO's extent is
    force_no_ambient: bool = False             # evaluate RenderScene's reference without the IBL samplers
    sky_state: tuple = (0, 0)                  # (m_updateEnvCubemapPattern, m_bIsDirty) of the Sky node in front of the frame
    sky_light: tuple = ()                      # SkyParams::lightDirection
    frame_start: object = None                 # the state in front of the frame's transfer list (name -> words): what the culls recorded there read
    ctx: object = None                         # a HipContext, for the one reference that is a C-ABI sequence (the cascade maps); None: that part is left out
    shadow_passes: tuple = ()                  # sceneView.m_shadowMapsToUpdate of this frame: dicts of cascade, shadow_type, dependencies, mask


@dataclass
class Expected:
    words: np.ndarray                 # flat, the resource's whole length: float32 or uint32
    mask: np.ndarray | None = None    # the words the reference determines (None: all)
    left_out: str = ""                # why the others are not
    rtol_mask: np.ndarray | None = None   # the float32 words held to |got - want| <= RADIANCE_RTOL |want| (no absolute floor; a non-finite word by its class)
    atol: float | None = None             # ... or, if given, to |got - want| < atol (the BRDF table)
    unchanged: bool = False               # the entry has nothing to do to this resource in this frame: not counted for liveness


def level0(fd, state, name):
    w, h, c, _ = fd.dims[name]
    a = state[name][:w * h * c].view(f32)
    return a.reshape(h, w, c) if c > 1 else a.reshape(h, w)


def prior(fd, state, name):
    """the resource in front of the entry; one the entry itself creates (absent there) counts as zeros of its length"""
    return state[name] if name in state else np.zeros(fd.words[name], np.uint32)


def with_level0(fd, state, name, image):
    out = state[name].copy().view(f32)
    w, h, c, _ = fd.dims[name]
    out[:w * h * c] = np.ascontiguousarray(image, f32).reshape(-1)
    return out


def same_bits_or_class(got, want):
    """finite float32 words by their bits, non-finite ones by class; integer words by their bits (eye_adaptation_ref.same_bits_or_class)"""
    from eye_adaptation_ref import same_bits_or_class as same
    if want.dtype != f32:
        return got.view(np.uint32) == want.view(np.uint32)
    return same(got.view(f32), want)


# ---- the references ------------------------------------------------------------------------------------------------------------------------------------
def ref_clear(entry):
    p, dst = entry.params, entry.params.target("target")

    def reference(before, fd):
        if dst == "DepthBuffer":   # ClearNode.cpp:93-101; the stencil has no storage on this path
            assert p.float("clearStencil") == 0
            return {dst: Expected(np.full(before[dst].size, f32(p.float("clearDepth")), f32))}
        w, h, c, _ = fd.dims[dst]
        return {dst: Expected(with_level0(fd, before, dst, np.broadcast_to(f32(p.vec4("clearColor")), (h, w, c))))}   # level 0 of a chain (:102-108)
    return reference


def ref_linearize(entry):
    src, dst = entry.params.target("depthStencil"), entry.params.target("target")

    def reference(before, fd):
        from oracle import oracle
        return {dst: Expected(oracle.linearize_depth(fd.frame.cameraZNearZFar[0], level0(fd, before, src)).reshape(-1))}
    return reference


def ref_light_culling(entry):
    src = entry.params.target("depthStencil")

    def reference(before, fd):
        from oracle import oracle
        from sailor_amd import host
        w, h, _, _ = fd.dims[src]
        lights = before["light"].view(np.uint8)[:fd.num_lights * host.LIGHT_DTYPE.itemsize].view(host.LIGHT_DTYPE)
        grid, indices, _ = oracle.light_cull(fd.frame, w, h, lights, level0(fd, before, src))
        want_grid = prior(fd, before, "lightsGrid").copy()
        want_grid[:grid.size] = grid.reshape(-1)
        grid_mask = np.zeros(want_grid.size, bool)
        grid_mask[:grid.size] = True
        want = prior(fd, before, "culledLights").copy()
        n = 1 + int(indices[0])
        want[:n] = indices[:n]
        mask = np.zeros(want.size, bool)
        mask[:n] = True
        return {"lightsGrid": Expected(want_grid, grid_mask, "the word behind the last tile's record belongs to nobody (LightCullingNode.cpp:64-65: + 1)"),
                "culledLights": Expected(want, mask, "the slots behind the listed indices hold what the allocation or an earlier frame left")}
    return reference


def ref_blit(entry):
    src, dst = entry.params.target("src"), entry.params.target("dst")

    def reference(before, fd):
        sw, sh, sc, _ = fd.dims[src]
        dw, dh, dc, _ = fd.dims[dst]
        assert sc == dc
        if sc == 1:   # a depth format on either side: Nearest (BlitNode.cpp:67,88)
            from hbao_ref import Ref32
            return {dst: Expected(with_level0(fd, before, dst, Ref32.blit(level0(fd, before, src), dw, dh)))}
        from effects_ref import Ref32
        return {dst: Expected(with_level0(fd, before, dst, Ref32.blit_linear(level0(fd, before, src), dw, dh)))}
    return reference


def ref_depth_highz(entry):
    src, dst = entry.params.target("src"), entry.params.target("dst")

    def reference(before, fd):
        from oracle import oracle
        w, h, _, levels = fd.dims[dst]
        return {dst: Expected(np.ascontiguousarray(oracle.hiz_build(level0(fd, before, src), w, h, levels), f32).reshape(-1))}
    return reference


HBAO_KEYS = ("occlusionRadius", "occlusionPower", "occlusionAttenuation", "occlusionBias", "noiseScale")
HBAO_BLUR_KEYS = ("sharpness", "distanceScale", "radius")
MOTION_BLUR_KEYS = ("intensity", "samples", "maxSpeed")


def ref_hbao(entry):
    p = entry.params
    assert p.string("defines") == ""
    dst, depth, noise = p.target("color"), p.target("depthSampler"), p.target("noiseSampler")
    assert noise == "g_noiseSampler"

    def reference(before, fd):
        from hbao_ref import Ref32
        w, h, _, _ = fd.dims[dst]
        values = {k: p.float("data." + k) for k in HBAO_KEYS}
        return {dst: Expected(with_level0(fd, before, dst, Ref32.hbao(fd.frame, level0(fd, before, depth), fd.noise, values, w, h)))}
    return reference


def ref_hbao_blur(entry):
    p = entry.params
    defines = p.string("defines").split()
    assert defines in (["VERTICAL"], ["HORIZONTAL"])
    dst, ao, depth = p.target("color"), p.target("aoSampler"), p.target("depthSampler")

    def reference(before, fd):
        from hbao_ref import Ref32
        w, h, _, _ = fd.dims[dst]
        values = {k: p.float("data." + k) for k in HBAO_BLUR_KEYS}
        return {dst: Expected(with_level0(fd, before, dst, Ref32.blur_pass(level0(fd, before, ao), level0(fd, before, depth), values, w, h, defines == ["VERTICAL"])))}
    return reference


def ref_bloom(entry):
    p = entry.params
    dst = p.target("bloom")

    def reference(before, fd):
        import bloom_ref
        _, _, _, levels = fd.dims[dst]
        chain = bloom_ref.bloom_chain(level0(fd, before, dst), levels, dirt=fd.dirt, threshold=p.vec4("threshold")[0], knee=p.vec4("knee")[0],
                                      bloom_intensity=p.vec4("bloomIntensity")[0], dirt_intensity=p.vec4("dirtIntensity")[0])
        return {dst: Expected(bloom_ref.flatten(chain))}
    return reference


def ref_eye_adaptation(entry):
    p = entry.params
    assert p.string("toneMappingShader") == "Shaders/Tonemapping.shader"
    dst, hdr, full = p.target("color"), p.target("hdrColor"), p.target("colorSampler")
    p.target("depthStencil")   # named by the entry, read by nothing in the node (EyeAdaptationNode.cpp)

    def reference(before, fd):
        import eye_adaptation_ref as ea
        from sailor_amd import host
        ops = sum({"ACES": ea.ACES, "UNCHARTED2": ea.UNCHARTED2, "LUMINANCE": ea.LUMINANCE}[d] for d in p.string("toneMappingDefines").split())
        assert hdr == full
        w, h, _, _ = fd.dims[hdr]
        c = host.eye_adaptation_constants(w, h, fd.delta_time)
        k = f32(c.minLog2Luminance), f32(c.invLog2LuminanceRange), f32(c.log2LuminanceRange), f32(c.numPixels), f32(c.timeCoeff)
        # the node clears its 1 x 1 target to 0.5 in the frame that creates it (EyeAdaptationNode.cpp:97); afterwards the state carries the last value
        last = f32(0.5) if fd.first_frame else prior(fd, before, "eyeAdaptation").view(f32)[fd.eye_luminance_word]
        _, lum, ldr = ea.step(ea.Ref32, level0(fd, before, hdr), last, fd.delta_time, ops, white_point=p.vec4("data.whitePoint")[:3], exposure=p.vec4("data.exposure")[0],
                              constants=k)
        state = prior(fd, before, "eyeAdaptation").copy()
        state[:256] = 0   # the average pass leaves the histogram zeroed for the next frame
        state[fd.eye_luminance_word] = f32(lum).view(np.uint32)
        mask = np.zeros(state.size, bool)
        mask[:256] = True
        mask[fd.eye_luminance_word] = True
        return {dst: Expected(with_level0(fd, before, dst, ldr)), "eyeAdaptation": Expected(state, mask, "words of the state that are neither a count nor the adapted luminance")}
    return reference


def ref_motion_blur(entry):
    p = entry.params
    assert p.string("defines") == ""
    dst, depth, color = p.target("color"), p.target("depthSampler"), p.target("colorSampler")

    def reference(before, fd):
        from tail_ref import Ref32
        w, h, _, _ = fd.dims[dst]
        values = {k: p.float("data." + k) for k in MOTION_BLUR_KEYS}
        return {dst: Expected(with_level0(fd, before, dst, Ref32.motion_blur(fd.frame, fd.previous, level0(fd, before, depth), level0(fd, before, color), values, w, h)))}
    return reference


def ref_debug_view(entry):
    p = entry.params
    dst, scene, linear = p.target("color"), p.target("ldrSceneSampler"), p.target("linearDepthSampler")

    def reference(before, fd):
        import tail_ref
        defines = p.string("defines").split()   # the shipped line is a YAML comment: the empty set, the scene copy
        assert len(defines) <= 1
        mode = {"": tail_ref.SCENE, "AO": tail_ref.AO, "LIGHT_TILES": tail_ref.LIGHT_TILES, "CASCADES": tail_ref.CASCADES}[defines[0] if defines else ""]
        w, h, _, _ = fd.dims[dst]
        tx, ty = (fd.width - 1) // 16 + 1, (fd.height - 1) // 16 + 1
        want = tail_ref.Ref32.debug_view(fd.frame, mode, w, h, scene=level0(fd, before, scene), linear_depth=level0(fd, before, linear),
                                         grid=before["lightsGrid"][:tx * ty * 2].reshape(-1, 2), culled=before["culledLights"], ao=level0(fd, before, "g_AO"))
        return {dst: Expected(with_level0(fd, before, dst, want))}
    return reference


def surface_scene(fd, tag):
    """the batches of one render queue as a surface_ref / masked_ref scene: every instance of them, in drawing order.  The GPU culls draw a subset; what
    they leave out has no fragment in the frame (the cull is conservative), so the planes and the depth are those of the whole queue"""
    s, draws = fd.scene, []
    for batch, t, flags in zip(s["batches"], s["tags"], s["flags"]):
        if t != tag:
            continue
        count, n, first_index, vertex_offset, first_instance = (int(x) for x in batch)
        draws.append(dict(vertices=s["vertices"][vertex_offset:], indices=s["indices"][first_index:first_index + count].reshape(-1, 3), instance_ids=None,
                          first_instance=first_instance, num_drawn=n, cull_back=not flags & 2, alpha_cutout=bool(flags & 1)))
    assert draws, tag
    return dict(W=fd.width, H=fd.height, view=np.array(list(fd.frame.view), f32), projection=np.array(list(fd.frame.projection), f32), instances=s["instances"],
                materials=s["materials"], textures=s["textures"], srgb=s["srgb"], draws=draws)


def indirect_commands(fd, tag):
    """the node's indirect commands as its cull on the transfer list leaves them: the host's records over the queue's batches packed in drawing order, then
    oracle.mesh_cull_compact against the pyramid the frame STARTED with (the last frame's: the transfer list executes before the first entry), as
    tests/test_indirect_runtime_gpu.py's oracle_counts"""
    from oracle import oracle
    s = fd.scene
    own = [b for b, t in zip(s["batches"], s["tags"]) if t in (tag, "")]
    packed = np.concatenate([s["instances"][int(b[4]):int(b[4]) + int(b[1])].view(np.uint8).reshape(-1, 96) for b in own]).reshape(-1).view(s["instances"].dtype)
    commands, at = np.zeros((len(own), 5), np.uint32), 0
    for j, b in enumerate(own):
        commands[j] = (b[0], b[1], b[2], b[3], at)
        at += int(b[1])
    w, h, _, levels = fd.dims["DepthHighZ"]
    _, after = oracle.mesh_cull_compact(fd.frame, packed, len(packed), 0, commands, hiz=(fd.frame_start["DepthHighZ"].view(f32), w, h, levels))
    return Expected(np.ascontiguousarray(after, np.uint32).reshape(-1))


def cascade_maps(before, fd):
    """(a) of tests/test_shadow_prepass_runtime_gpu.py: every cascade this frame re-renders through the C-ABI sequence -- sailor_hip_raster_depth over the ids of
    the pass's caster mask, batch by batch, back faces culled; sailor_hip_shadow_resolve; sailor_hip_evsm_blur (2, 5) for an EVSM pass -- over the host's
    cascade matrix; a cascade without a pass must keep its bits.  The masks are the ones LightingECS planned (its planning is tests/test_shadow_prepass_cpu.py's)."""
    import torch
    from sailor_amd import _lib, host
    from sailor_amd.forward_plus import evsm_blur, raster_depth, shadow_resolve
    ctx, s = fd.ctx, fd.scene
    lm = host.csm_matrices(fd.light_view, fd.camera.world, fd.camera.aspect, fd.camera.fov, fd.camera.z_near, fd.camera.z_far)
    positions = torch.from_numpy(np.ascontiguousarray(s["vertices"][:, 2:5])).to(ctx.device)
    indices = torch.from_numpy(s["indices"].view(np.int32)).to(ctx.device)
    models = torch.from_numpy(np.ascontiguousarray(s["instances"]["model"])).to(ctx.device)
    by_cascade = {p["cascade"]: p for p in fd.shadow_passes}
    out = {}
    for k, name in enumerate(CASCADES):
        if k not in by_cascade:
            out[name] = Expected(before[name].copy(), unchanged=True)
            continue
        p = by_cascade[k]
        evsm = p["shadow_type"] == 2
        mask = np.array(p["mask"], np.uint64)
        for d in p["dependencies"]:   # m_internalCommandsList: the node draws those passes' casters into this map as well
            mask = mask | np.array(fd.shadow_passes[d]["mask"], np.uint64)
        ids = np.nonzero(np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:len(s["instances"])])[0].astype(np.uint32)
        size = int(round(np.sqrt(before[name].size / 4))) if evsm else int(round(np.sqrt(before[name].size * 2)))
        depth = torch.zeros((size, size), dtype=torch.float32, device=ctx.device)
        for count, n, first_index, vertex_offset, first_instance in (tuple(int(x) for x in b) for b in s["batches"]):
            own = ids[(ids >= first_instance) & (ids < first_instance + n)]
            if len(own):
                raster_depth(ctx, lm[k], positions[vertex_offset:], indices[first_index:first_index + count], models, size, size,
                             instance_ids=torch.from_numpy(own.view(np.int32)).to(ctx.device), depth=depth, cull_back=True)
        image = shadow_resolve(ctx, depth, _lib.SHADOWMAP_RGBA32F if evsm else _lib.SHADOWMAP_R16F)
        if evsm:
            evsm_blur(ctx, image, 2, 5, torch.empty_like(image))
        ctx.synchronize()
        out[name] = Expected(image.cpu().numpy().reshape(-1).view(np.uint8).view(np.uint32).copy())
    return out


def ref_depth_prepass(entry):
    p = entry.params
    depth = p.target("depthStencil")
    p.target("depthHighZ")   # what the cull on the transfer list tests against (the last frame's pyramid): no fragment depends on it

    def reference(before, fd):
        import masked_ref
        assert p.flag("GPUCulling")
        seed = None if p.flag("ClearDepth") else level0(fd, before, depth)   # ClearDepth: the pass begins from cleared keys
        out = masked_ref.render(surface_scene(fd, p.string("Tag")), prepass=seed)
        return {depth: Expected(with_level0(fd, before, depth, out["depth"])), f"indirect{entry.index}": indirect_commands(fd, p.string("Tag"))}
    return reference


def ref_render_scene(entry):
    p = entry.params
    color, depth = p.target("color"), p.target("depthStencil")
    p.target("depthHighZ")

    def reference(before, fd):
        import masked_ref
        from oracle import oracle
        from sailor_amd import host
        assert p.flag("GPUCulling")
        w, h = fd.width, fd.height
        out = masked_ref.render(surface_scene(fd, p.string("Tag")), prepass=level0(fd, before, depth))
        lights = before["light"].view(np.uint8)[:fd.num_lights * host.LIGHT_DTYPE.itemsize].view(host.LIGHT_DTYPE)
        tx, ty = host.num_tiles(w, h)
        maps = []
        for k, name in enumerate(CASCADES):   # cascade 0 of an EVSM light holds four moments, the others one fp16 depth (LightingECS.cpp:53-63)
            raw = before[name]
            side = int(round(np.sqrt(raw.size / 4))) if k == 0 else int(round(np.sqrt(raw.size * 2)))
            maps.append(raw.view(f32).reshape(side, side, 4) if k == 0 else raw.view(np.float16).reshape(side, side))
        csm, keep = oracle.make_csm(before["lightsMatrices"].view(f32).reshape(4, 16), maps)
        ibl = None
        if all(n in before for n in IBL_SAMPLERS) and not fd.force_no_ambient:
            irr = before["g_irradianceCubemap"].view(f32)
            irr_size = int(round(np.sqrt(irr.size / 24)))
            env, env_size, env_levels = before["g_envCubemap"].view(f32), 256, 8
            assert env.size == sum(6 * max(1, env_size >> l) ** 2 * 4 for l in range(env_levels))
            lut = before["g_brdfSampler"].view(f32)
            lut_side = int(round(np.sqrt(lut.size / 2)))
            # g_AO reaches the shade only when its extent is the frame's ("HBAO": the shipped file declares it ViewportWidth squared, a kept
            # simplification): on any other viewport the pass shades with ao = 1.  Pinned here as it is.
            aw, ah, _, _ = fd.dims["g_AO"]
            ao = level0(fd, before, "g_AO") if (aw, ah) == (w, h) and not fd.force_ao_one else None
            ibl, keep2 = oracle.make_ibl(irr.reshape(6, irr_size, irr_size, 4), env, env_size, env_levels, lut.reshape(lut_side, lut_side, 2), ao)
        radiance = oracle.shade(fd.frame, w, h, out["planes"], lights, before["lightsGrid"][:tx * ty * 2].reshape(-1, 2), before["culledLights"], csm, ibl=ibl)
        covered = out["covered"]
        main = level0(fd, before, color).copy()
        main[covered] = radiance[covered]   # sailor_hip_surface_composite: target = covered ? radiance : target
        want = with_level0(fd, before, color, main)
        held = np.zeros(want.size, bool)
        held[:w * h * 4] = np.repeat(covered.reshape(-1), 4)
        return {color: Expected(want, rtol_mask=held), f"indirect{entry.index}": indirect_commands(fd, p.string("Tag"))}
    return reference


@functools.lru_cache(maxsize=8)
def _sky_planes(frame_bytes, light, w, h):
    import sky_cases
    import sky_ref
    from sailor_amd import _lib
    r = sky_ref.Ref32()
    U = sky_cases.frame_uniforms(r, _lib.UboFrameData.from_buffer_copy(frame_bytes), list(light))
    return r.compose(U, r.fill(U, sky_ref.SKY_RESOLUTION, sky_ref.SKY_RESOLUTION), r.sun(U, sky_ref.SUN_RESOLUTION, sky_ref.SUN_RESOLUTION), w, h)


@functools.lru_cache(maxsize=8)
def _sky_face(face, position, light):
    import sky_cases
    import sky_ref
    r = sky_ref.Ref32()
    return r.env_face(sky_cases.face_uniforms(r, face, list(position), list(light)), SKY_CUBE_SIZE)


def ref_sky(entry):
    p = entry.params
    color = p.target("color")
    p.target("linearDepth")   # read by the cloud march and the sun shafts only: neither is drawn without their textures and shaders

    def reference(before, fd):
        """the node without cloud textures, star mesh or the opt-in shaders: FILL, SUN and COMPOSE into `color` every frame (tests/test_sky_runtime_gpu.py's
        restatement and bound), and while the node is dirty one face of g_skyCubemap a frame"""
        w, h, _, _ = fd.dims[color]
        image = _sky_planes(bytes(fd.frame), tuple(fd.sky_light), w, h)
        out = {color: Expected(with_level0(fd, before, color, image), rtol_mask=np.ones(before[color].size, bool))}
        pattern, dirty = fd.sky_state
        if not dirty:
            out["g_skyCubemap"] = Expected(before["g_skyCubemap"].copy(), unchanged=True)
            return out
        assert pattern < 6, "the two mip-generation frames of the bake are not restated"
        cube = prior(fd, before, "g_skyCubemap").copy().view(f32)
        face_words = SKY_CUBE_SIZE * SKY_CUBE_SIZE * 4
        cube[pattern * face_words:(pattern + 1) * face_words] = np.ascontiguousarray(_sky_face(pattern, tuple(float(x) for x in fd.camera.world[12:15]), tuple(fd.sky_light)), f32).reshape(-1)
        held = np.zeros(cube.size, bool)
        held[pattern * face_words:(pattern + 1) * face_words] = True
        mask = held if "g_skyCubemap" not in before else None   # a cube created in this frame: the other faces and the mips hold what the allocation held
        out["g_skyCubemap"] = Expected(cube, mask, "faces and mip levels of the new cube that no frame has written yet" if mask is not None else "", rtol_mask=held)
        return out
    return reference


def ref_environment(entry):
    def reference(before, fd):
        """What the captured frames hold of the node: the BRDF table it creates in the graph's first frame (the C oracle at tests/test_ambient_gpu.py's bound) and
        that it leaves its three samplers alone while it is not dirty.  The bake itself runs in the frame in which the Sky node's cube bake ends; a float64
        restatement of it at the shipped sizes (a 256 x 256 x 6 cube of 8 levels at 1 024 samples a texel, 32 x 32 x 6 texels of irradiance at 65 536) takes
        minutes and the shipped file has no knob for the sizes, so that frame is not captured."""
        from oracle import oracle
        out = {}
        for name in IBL_SAMPLERS:
            if name in before:
                out[name] = Expected(before[name].copy(), unchanged=True)
        if "g_brdfSampler" not in before:
            side = int(round(np.sqrt(fd.words["g_brdfSampler"] / 2)))
            lut = np.ascontiguousarray(oracle.compute_brdf_lut(side, side), f32).reshape(-1)
            out["g_brdfSampler"] = Expected(lut, rtol_mask=np.ones(lut.size, bool), atol=BRDF_ATOL)
        return out
    return reference


def ref_debug_draw(entry):
    color, depth = entry.params.target("color"), entry.params.target("depthStencil")

    def reference(before, fd):
        import lines_ref
        from sailor_amd import host
        w, h, _, _ = fd.dims[color]
        vertices = np.ascontiguousarray(fd.debug_vertices).view(np.uint8).view(lines_ref.VERTEX).reshape(-1)
        scene = dict(W=w, H=h, vp=host.mat4_mul(np.array(list(fd.frame.projection), f32), np.array(list(fd.frame.view), f32)), vertices=vertices, indices=None, prim_base=0,
                     depth=level0(fd, before, depth), target=level0(fd, before, color))
        out = lines_ref.render(scene)
        return {color: Expected(with_level0(fd, before, color, out["target"])), depth: Expected(with_level0(fd, before, depth, out["depth"]))}
    return reference


def ref_ui(entry):
    color = entry.params.target("color")
    entry.params.target("depthStencil")   # the pass's depth attachment: bound, neither tested nor written (ImGuiUI.shader has no depth state)

    def reference(before, fd):
        import ui_ref
        w, h, _, _ = fd.dims[color]
        flat, atlas = fd.ui
        assert (flat["width"], flat["height"]) == (w, h)
        s = dict(W=w, H=h, vertices=flat["vertices"], indices=flat["indices"], index_bytes=2, commands=flat["commands"], scale=flat["scale"], translate=flat["translate"],
                 texture=atlas, target=level0(fd, before, color))
        return {color: Expected(with_level0(fd, before, color, ui_ref.render(s)["target"]))}
    return reference


def ref_shadow_matrices(entry):
    def reference(before, fd):
        """(b) of tests/test_shadow_prepass_runtime_gpu.py: the host's cascade matrices x light matrix, for the cascades this frame re-renders; the maps -- (a),
        the C-ABI sequence -- are not restated here yet"""
        from sailor_amd import host
        want = before["lightsMatrices"].copy().view(f32).reshape(4, 16)
        lm = host.csm_matrices(fd.light_view, fd.camera.world, fd.camera.aspect, fd.camera.fov, fd.camera.z_near, fd.camera.z_far)
        for k in fd.shadow_cascades:
            want[k] = lm[k]
        out = {"lightsMatrices": Expected(want.reshape(-1))}
        if fd.ctx is not None:   # (the C-ABI sequence needs the device)
            out.update(cascade_maps(before, fd))
        return out
    return reference


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Stage:
    index: int
    name: str
    label: str
    params: Params
    roles: dict
    reads: tuple
    writes: tuple
    reference: object = None   # None: PENDING
    bound: str = BITS
    note: str = ""


LIGHTS_SET = ("light", "lightsMatrices") + LIST_BUFFERS + CASCADES + IBL_SAMPLERS


def _stage(entry: Entry) -> Stage:
    p, r = entry.params, entry.roles
    mk = lambda label, reads, writes, reference=None, note="": Stage(entry.index, entry.name, label, p, r, tuple(reads), tuple(writes), reference,
                                                                     BOUNDS.get(entry.name, BITS), note)
    if entry.name == "Clear":
        return mk(f"Clear {r['target']}", (), (r["target"],), ref_clear(entry))
    if entry.name == "DepthPrepass":
        tag = p.string("Tag")
        return mk(f"DepthPrepass {tag}", (r["depthStencil"], r["depthHighZ"], f"indirect{entry.index}"), (r["depthStencil"], f"indirect{entry.index}"),
                  ref_depth_prepass(entry))
    if entry.name == "LinearizeDepth":
        return mk("LinearizeDepth", (r["depthStencil"],), (r["target"],), ref_linearize(entry))
    if entry.name == "LightCulling":
        return mk("LightCulling", (r["depthStencil"], "light"), LIST_BUFFERS, ref_light_culling(entry))
    if entry.name == "ShadowPrepass":
        return mk("ShadowPrepass", (), CASCADES + ("lightsMatrices",), ref_shadow_matrices(entry))
    if entry.name == "Sky":
        return mk("Sky", (r["linearDepth"], "g_noiseSampler"), (r["color"], "g_skyCubemap"), ref_sky(entry), note="the two mip-generation frames of the bake are not captured")
    if entry.name == "Environment":
        return mk("Environment", ("g_skyCubemap",), IBL_SAMPLERS, ref_environment(entry), note="the BRDF table and idleness; the bake's frame is not captured")
    if entry.name == "Blit":
        return mk(f"Blit {r['src']} -> {r['dst']}", (r["src"],), (r["dst"],), ref_blit(entry))
    if entry.name == "DepthHighZ":
        return mk("DepthHighZ", (r["src"],), (r["dst"],), ref_depth_highz(entry))
    if entry.name == "RenderScene":
        tag = p.string("Tag")
        # g_AO reaches the shade only when its extent is the frame's ("HBAO": the shipped file declares it ViewportWidth squared, a kept
        # simplification): on a non-square viewport the pass shades with ao = 1.  It is listed as read either way.
        # The Masked pass ends by storing its depth into the attachment (a pass that held a cutout draw): over the prepass's depth those are the same bits, so
        # the attachment is NOT among the writes and the stray-write check holds the pass to that.
        return mk(f"RenderScene {tag}", (r["color"], r["depthStencil"], r["depthHighZ"], "g_AO", f"indirect{entry.index}") + LIGHTS_SET, (r["color"], f"indirect{entry.index}"),
                  ref_render_scene(entry))
    if entry.name == "DebugDraw":
        return mk("DebugDraw", (r["color"], r["depthStencil"]), (r["color"], r["depthStencil"]), ref_debug_draw(entry))
    if entry.name == "Bloom":
        return mk("Bloom", (r["bloom"], "g_lensDirtSampler"), (r["bloom"],), ref_bloom(entry))
    if entry.name == "EyeAdaptation":
        return mk("EyeAdaptation", (r["hdrColor"], r["colorSampler"], r["depthStencil"], "eyeAdaptation"), (r["color"], "eyeAdaptation"), ref_eye_adaptation(entry))
    if entry.name == "RenderImGui":
        return mk("RenderImGui", (r["color"], r["depthStencil"]), (r["color"],), ref_ui(entry))
    if entry.name == "PostProcess":
        shader = p.string("shader")
        inputs = tuple(v for k, v in r.items() if k != "color")
        if shader == "Shaders/HBAO.shader":
            return mk("HBAO", inputs, (r["color"],), ref_hbao(entry))
        if shader == "Shaders/HBAO_Blur.shader":
            return mk(f"HBAO_Blur {p.string('defines')}", inputs, (r["color"],), ref_hbao_blur(entry))
        if shader == "Shaders/MotionBlur.shader":
            return mk("MotionBlur", inputs, (r["color"],), ref_motion_blur(entry))
        if shader == "Shaders/Debug.shader":
            return mk("Debug", inputs + LIST_BUFFERS + ("g_AO",), (r["color"],), ref_debug_view(entry))
    raise ValueError(f"entry {entry.index} ({entry.name}) has no stage")


def stages(text: str | None = None):
    """(targets, the stages of the text, in file order); the shipped text unless another is given"""
    targets, entries = parse(shipped_text() if text is None else text)
    return targets, [_stage(e) for e in entries]


# the entries whose reference is still missing (by index in the shipped file): pinned, so that the set can only shrink on purpose
PENDING = ()
# of a stage that has a reference, the writes that reference does not determine yet
PARTLY_PENDING = {}


def transfer_writes(table):
    """what the nodes record into the frame's TRANSFER list, which executes as a whole before the first entry: the culls' indirect commands, and in the
    graph's first frame the EyeAdaptation node's histogram initialisation"""
    return tuple(f"indirect{s.index}" for s in table if s.name in ("DepthPrepass", "RenderScene") and s.params.flag("GPUCulling")) + ("eyeAdaptation",)


def ui_draw_data(width, height):
    """one small ImGui list from ui_cases' builder: a translucent panel, a glyph quad under a tighter clip rectangle"""
    import ui_cases
    from sailor_amd import host
    a = ui_cases.dl().clip(0, 0, width, height).rect(3, 2, width * 0.6, height * 0.5, ui_cases.HALF_RED)
    a.clip(4.5, 3.5, width * 0.5, height * 0.4).quad(5, 4, 21, 20, (0.25, 0.25), (0.75, 0.75), host.ui_color(1, 1, 0.9, 0.9))
    return host.ui_draw_data([a], (float(width), float(height)))


def capture_names(targets, table):
    """every name a captured frame must hold (the issue's list, and the nodes' indirect commands)"""
    return tuple(targets) + PER_FRAME_TARGETS + LIST_BUFFERS + ("light", "lightsMatrices") + CASCADES + IBL_SAMPLERS + ("g_skyCubemap", "eyeAdaptation") + \
        transfer_writes(table)[:-1]
