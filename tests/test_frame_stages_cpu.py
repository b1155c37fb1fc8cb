"""tests/frame_stages.py without a device: the table has exactly the shipped file's entries in order and agrees with FrameGraphAsset::Deserialize on what the
text declares; every role under an entry's `renderTargets:` is read or written by its stage and every output role is written; every parameter line of an entry
that has a reference is consumed when that reference runs (over a small synthetic state); the entries without a reference are exactly the pinned PENDING set."""
import re

import numpy as np
import pytest

import frame_stages as fs
from sailor_amd import _lib, host, synth
from sailor_amd.runtime_binding import parse_renderer
from test_default_renderer_gpu import frame_entries

f32 = np.float32
W, H = 48, 32   # small and not square: the references only have to run here


@pytest.fixture(scope="module")
def table():
    return fs.stages()


def test_the_table_has_the_shipped_entries_in_order(table):
    targets, stages = table
    text = fs.shipped_text()
    assert [s.name for s in stages] == frame_entries(text) and len(stages) == 23
    assert [s.index for s in stages] == list(range(23))
    n, summary = parse_renderer(text, 128, 96)
    assert n == len(stages)
    # the labels tell the like-named entries apart
    assert len({s.label for s in stages}) == len(stages), [s.label for s in stages]


def test_the_text_parse_agrees_with_the_runtimes_parser(table):
    """the same file through FrameGraphAsset::Deserialize: every target's extent and mip count at two viewports, every entry's parameter lines"""
    targets, stages = table
    text = fs.shipped_text()
    for w, h in ((128, 96), (96, 96), (W, H)):
        _, summary = parse_renderer(text, w, h)
        declared = dict((t.split(":")[0], t.split(":")) for t in summary.split(";")[0][len("targets="):].split(","))
        dims = fs.target_dims(targets, w, h)
        assert set(declared) == set(dims)
        for name, (tw, th, channels, levels) in dims.items():
            assert declared[name][1] == f"{tw}x{th}" and int(declared[name][3]) == levels, (name, declared[name], dims[name])
            assert (channels == 4) == declared[name][2].startswith("R16G16B16A16"), name
    nodes = re.findall(r"(\w+)\[(\w*)\]\{([^}]*)\}", summary.split(";nodes=")[1].split(";values=")[0])
    assert len(nodes) == len(stages)
    for (name, tag, body), s in zip(nodes, stages):
        assert name == s.name
        got = {}
        for item in filter(None, body.split(";")):
            section, rest = item.split(" ", 1)
            key, value = rest.split("=", 1)
            got[({"rt": "renderTargets"}.get(section, section), key)] = value
        mine = dict(s.params.lines)
        assert set(got) == set(mine), (s.label, set(got) ^ set(mine))
        for k, v in got.items():
            if k[0] == "float":
                assert float(v) == float(mine[k]), (s.label, k)
            elif k[0] == "vec4":
                assert [float(x) for x in v.split()] == [float(x) for x in mine[k].strip("[]").split(",")], (s.label, k)
            else:
                assert v in (mine[k], "~" if mine[k] == "" else mine[k]) or (mine[k] == "" and v.startswith("#")), (s.label, k, v, mine[k])


def test_every_role_is_read_or_written_and_every_output_role_is_written(table):
    _, stages = table
    for s in stages:
        for role, name in s.roles.items():
            assert name in s.reads or name in s.writes, (s.label, role, name)
            if role in fs.OUTPUT_ROLES:
                assert name in s.writes, (s.label, role, name)
        assert s.writes, s.label
        if s.reference is not None:
            assert s.bound == fs.BOUNDS.get(s.name, fs.BITS)


def test_the_entries_without_a_reference_are_the_pinned_set(table):
    _, stages = table
    assert tuple(s.index for s in stages if s.reference is None) == fs.PENDING
    assert all(s.note.startswith("PENDING") for s in stages if s.reference is None)
    assert fs.PARTLY_PENDING == {}
    assert fs.PENDING == ()
    assert fs.transfer_writes(stages) == ("indirect1", "indirect2", "indirect15", "indirect16", "eyeAdaptation")


def synthetic(targets, stages):
    """a state of the right shapes (random, finite) and the frame data of a camera over it: enough for every reference to run"""
    rng = np.random.default_rng(11)
    dims = fs.target_dims(targets, W, H)
    dims["BackBuffer"], dims["DepthBuffer"] = (W, H, 4, 1), (W, H, 1, 1)
    state = {name: rng.uniform(0.05, 0.95, fs.chain_words(*d)).astype(f32).view(np.uint32) for name, d in dims.items()}
    tx, ty = host.num_tiles(W, H)
    state["lightsGrid"] = np.zeros(tx * ty * 2 + 1, np.uint32)
    state["culledLights"] = np.zeros(tx * ty * fs.LIGHTS_PER_TILE + 1, np.uint32)
    lights = synth.make_frame("tiny", with_surface=False).lights[:8]
    state["light"] = np.ascontiguousarray(lights).view(np.uint8).view(np.uint32).copy()
    state["lightsMatrices"] = np.zeros(64, np.uint32)
    for k, name in enumerate(fs.CASCADES):   # cascade 0: four fp32 moments a texel; the others: one fp16 depth
        state[name] = rng.uniform(0, 1, 16 * 16 * (4 if k == 0 else 1)).astype(f32 if k == 0 else np.float16).view(np.uint32)
    for name in fs.transfer_writes(stages)[:-1]:
        state[name] = np.zeros(5 * (2 if name in ("indirect1", "indirect15") else 1), np.uint32)   # two Opaque batches, one Masked
    state["g_skyCubemap"] = np.zeros(96, np.uint32)   # (the Sky node is not dirty here: it leaves the cube alone, whatever its size)
    state["eyeAdaptation"] = np.zeros(260, np.uint32)
    state["eyeAdaptation"][256] = f32(0.4).view(np.uint32)
    from test_shipped_frame_gpu import camera, scene_arrays
    cam = camera(W, H)
    moved = synth.make_camera(W, H, z_far=1000.0)
    moved.world = host.transform_matrix([0.5, 1.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0])
    previous = host.fill_frame_data(moved.world, cam.fov, cam.z_near, cam.z_far, W, H)
    vertices = np.zeros(2, _lib.VERTEX_P3C4_DTYPE)
    vertices["position"] = [(-5, 0, -20), (5, 2, -30)]
    vertices["color"] = (1, 0.5, 0, 1)
    import ui_cases
    fd = fs.FrameData(W, H, cam.frame, previous, 1.0 / 60.0, False, dims, num_lights=len(lights), noise=rng.uniform(0, 1, (4, 4, 4)).astype(f32),
                      dirt=rng.uniform(0, 1, (8, 8, 4)).astype(f32), eye_luminance_word=256, debug_vertices=vertices,
                      ui=(host.ui_flatten(fs.ui_draw_data(W, H)), ui_cases.ATLAS), camera=cam, light_view=np.eye(4, dtype=f32).reshape(-1), shadow_cascades=(0, 1, 2, 3), scene=scene_arrays(), sky_state=(8, 0), frame_start=state,
                      sky_light=tuple(host.sky_params().lightDirection), words={"g_brdfSampler": 16 * 16 * 2})
    return state, fd


def test_every_parameter_line_is_consumed_by_its_reference(table):
    targets, stages = fs.stages()   # a fresh table: the look-ups of this test alone
    state, fd = synthetic(targets, stages)
    for s in stages:
        if s.reference is None:
            continue
        out = s.reference(state, fd)
        # (without a device: the cubes the Environment node has not created are no writes of this frame, the cascade maps' C-ABI sequence is left out)
        absent = {"Environment": {"g_irradianceCubemap", "g_envCubemap"}, "ShadowPrepass": set(fs.CASCADES)}.get(s.name, set())
        assert set(out) == set(s.writes) - absent, (s.label, sorted(out), s.writes)
        for name, e in out.items():
            size = state[name].size if name in state else fd.words[name]   # (a resource the entry creates)
            assert e.words.size == size and e.words.dtype.itemsize == 4, (s.label, name, e.words.size, size)
            assert e.mask is None or (e.mask.shape == e.words.shape and e.mask.any() and e.left_out), (s.label, name)
            assert e.rtol_mask is None or (e.rtol_mask.shape == e.words.shape and s.name in ("RenderScene", "Sky", "Environment")), (s.label, name)
        assert s.params.unused() == [], (s.label, s.params.unused())


def test_a_parameter_no_reference_reads_is_reported():
    """the tracking itself: a line added to an entry shows up as unused"""
    text = fs.shipped_text().replace("  - data.samples: 10\n", "  - data.samples: 10\n  - data.unheard: 3\n")
    targets, stages = fs.stages(text)
    state, fd = synthetic(targets, stages)
    blur = next(s for s in stages if s.label == "MotionBlur")
    blur.reference(state, fd)
    assert blur.params.unused() == [("float", "data.unheard")]
