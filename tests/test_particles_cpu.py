"""ExperimentalParticles without a GPU: the fp32 restatement of tests/particles_ref.py against its float64 form on every case (where the bounds of the GPU
test are measured), what each case reaches, the C-ABI's structs and symbols, the host mirror's registry, the fixtures."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import particles_cases as cases
import particles_ref as ref
from sailor_amd import _lib, host

ROOT = Path(__file__).resolve().parents[1]
f32, f64 = np.float32, np.float64


def both(c):
    return ref.update(c["records"], c["pc"], c["time"], f32), ref.update(c["records"], c["pc"], c["time"], f64)


def test_fp32_update_against_float64():
    """E_REF_MATRIX / E_REF_COLOUR of tests/particles_ref.py: the worst deviation over the generic instances of every case"""
    worst_m = worst_c = 0.0
    generic = 0
    for name, build in list(cases.UPDATE_CASES.items()) + [("pass_scene", cases.pass_scene)]:
        o32, o64 = both(build())
        g = ref.generic(o64)
        generic += int(g.sum())
        if g.any():
            worst_m = max(worst_m, ref.deviation(o32["model"][g], o64["model"][g]).max())
            worst_c = max(worst_c, ref.deviation(o32["color"][g], o64["color"][g]).max(), ref.deviation(o32["colorOld"][g], o64["colorOld"][g]).max())
        # the discrete steps are the same in both forms
        for k in ("i_new", "i_old", "isCulled", "current"):
            np.testing.assert_array_equal(o32[k], o64[k], err_msg=f"{name}: {k}")
    print(f"E_ref over {generic} generic instances: matrix {worst_m:.3f}, colour {worst_c:.3f} (x 2^-23 x the largest magnitude)")
    assert generic > 1200
    # the constants ARE the measurement: within the stated allowance above and below
    assert ref.E_MEASURED_MATRIX / ref.LIBM_ALLOWANCE <= worst_m <= ref.E_REF_MATRIX
    assert ref.E_MEASURED_COLOUR / ref.LIBM_ALLOWANCE <= worst_c <= ref.E_REF_COLOUR


def test_update_cases_reach_what_they_are_there_for():
    o = {name: ref.update(*(lambda c: (c["records"], c["pc"], c["time"]))(build())) for name, build in cases.UPDATE_CASES.items()}
    # U1: frame 3 keeps every index in range; frame 0 wraps every old record and every current > 0 new record to the zero record
    a, b = o["U1_frame3"], o["U1_frame0"]
    assert a["frame"] == 3 and not a["zero_new"].any() and not a["zero_old"].any() and len(a["current"]) == 15
    assert b["frame"] == 0 and b["zero_old"].all() and (b["zero_new"] == (b["current"] > 0)).all() and (b["current"] > 0).sum() == 10
    assert (b["i_old"] >= (2 ** 32 - 45) // 3).all()                           # (0 - current - 1) * 15 wrapped, then / 3: not clamped to 0
    zero = b["zero_new"]
    assert (b["model"][zero] == np.array([0] * 15 + [1], f32)).all()            # the zero record: an all-zero scale
    # U2
    assert len(o["U2_257"]["current"]) == 257 and len(o["U2_1000"]["current"]) == 1000
    # U3: +up, -up, one ulp off up, along x, along y, p1 == p2
    p = o["U3_placed"]
    assert p["gate"].tolist() == [False, False, True, True, True, False]
    ident = np.eye(4, dtype=f32).reshape(16)[[0, 1, 2, 4, 5, 6, 8, 9, 10]]
    for k in (0, 1, 2, 5):                                                     # the identity rotation: model = translate * scale exactly (-up is not flipped)
        rot = p["model"][k][[0, 1, 2, 4, 5, 6, 8, 9, 10]]
        scale = np.array([p["model"][k][0], p["model"][k][5], p["model"][k][10]], f32)
        assert (rot == ident * np.repeat(scale, 3)).all(), k
    assert np.isnan(p["angle"][5]) and p["dist"][5] == 0 and p["model"][5][10] == 0 and p["model"][5][0] == f32(0.5) * f32(1.5)
    assert p["model"][1][10] == 2 and p["angle"][1] == f32(np.pi)             # -up: rotation skipped although the angle is pi
    assert (p["model"][:, 12:16] == np.array([[1, 2, 4, 1], [1, 2, 2, 1], [p["model"][2][12], 2, 4, 1], [1.75, 2, 3, 1], [1, 2.75, 3, 1], [1, 2, 3, 1]], f32)).all()
    # U4: the compare is > 0.5
    assert o["U4_enabled"]["isCulled"].tolist() == [0, 0, 1, 1] and o["U4_enabled"]["enabled_margin"].min() == 0
    # U5
    assert o["U5_at_the_end"]["frame"] == 0 and o["U5_one_ulp_below"]["frame"] == 3
    # U6: current up to 7, the decay exact for 1 and 0.5
    for name, d in (("U6_decay_1", 1.0), ("U6_decay_half", 0.5)):
        assert o[name]["current"].max() == 7 and (o[name]["decay"] == f32(d) ** o[name]["current"].astype(f32)).all()


def test_the_golden_indices():
    g = np.load(ROOT / "tests" / "golden" / "tiny_particles.npz")
    n, frames, fps, tf = (int(v) for v in g["constants"])
    records = np.ascontiguousarray(g["records"]).view(ref.RECORD_DTYPE).reshape(-1)
    pc = host.particles_constants(n // tf, frames, fps, tf, float(g["trace_decay"]))
    assert pc.numInstances == n == 15 and len(records) == 20
    for frame in (3, 0):
        o = ref.update(records, pc, f32(frame))
        for k, key in (("i_new", "i_new"), ("i_old", "i_old"), ("zero_new", "zero_new"), ("zero_old", "zero_old"), ("isCulled", "is_culled")):
            np.testing.assert_array_equal(o[k].astype(g[f"frame{frame}_{key}"].dtype), g[f"frame{frame}_{key}"], err_msg=f"frame {frame}: {k}")


@pytest.fixture(scope="module")
def passes():
    s = cases.pass_scene()
    inst = ref.apply_update(s["before"], ref.update(s["records"], s["pc"], s["time"]))
    smap = ref.raster(inst["model"], s["vertices"], s["indices"], cases.MAP_W, cases.MAP_H, light_matrix=s["light_matrix"])
    pre = cases.prepass_depth(s, inst, ref)
    colour = ref.raster(inst["model"], s["vertices"], s["indices"], cases.W, cases.H, projection=s["projection"], view=s["view"], depth0=pre)
    args = (colour, inst, s["vertices"], s["lights"]["direction"][0], s["light_matrix"], s["projection"], s["view"], smap["map"], s["main0"])
    return dict(scene=s, inst=inst, smap=smap, pre=pre, colour=colour, r32=ref.shade(*args, T=f32), r64=ref.shade(*args, T=f64))


def test_the_pass_scene_reaches_every_branch(passes):
    s, inst, smap, colour, r = passes["scene"], passes["inst"], passes["smap"], passes["colour"], passes["r64"]
    assert (inst["materialInstance"] == 3).all() and (inst["_pad"] == 0).all()        # what the host built and the update leaves
    assert (inst["model"][2] == np.array([0] * 15 + [1], f32)).all()                     # the zero record
    m = smap["stats"]
    # order over depth: texels where a LATER primitive wrote a FARTHER (smaller) depth over an earlier one, and the map holds it
    assert m["later_farther"] >= 40 and m["z_outside"] > 0 and m["culled"] > 0 and m["degenerate"] >= 12 and m["large"] > 0
    under = (smap["owner"] != 0) & ((smap["owner"].astype(int) - 1) // 24 == 1)
    top0, top1 = f32(0.05) * f32(3) + f32(0.5), f32(0.05) * f32(-1.5) + f32(0.5)
    assert under.sum() > 80 and np.allclose(smap["map"][under], top1, atol=1e-6) and not np.isclose(smap["map"], top0, atol=1e-3).any()
    assert (smap["map"][smap["owner"] == 0] == 0).all() and (smap["owner"] == 0).sum() > 3000
    c = colour["stats"]
    assert c["cut_one"] > 0 and c["cut_two"] > 0 and c["culled"] > 0 and c["ties"] >= 12 and c["depth_failed"] >= 20 and c["large"] > 0
    tie = (colour["owner"] != 0) & ((colour["owner"].astype(int) - 1) // 24 == cases.TIE_CUBE)
    assert tie.sum() >= 12 and (colour["depth"][tie] == passes["pre"][tie]).all()
    cov = r["covered"]
    counts = {k: int((r[k] & cov).sum()) for k in ("early", "early_y", "early_z", "clamped", "dot_negative", "min_is_shadow", "floor_taken")}
    print(counts, "covered", int(cov.sum()), "lit taps", np.bincount(r["lit_taps"][cov & ~r["early"]].astype(int), minlength=17).tolist())
    assert cov.sum() > 200
    assert counts["early_y"] > 20 and counts["early_z"] > 5 and counts["clamped"] > 3
    taps = r["lit_taps"][cov & ~r["early"]]
    assert (taps == 16).sum() > 30 and (taps < 8).sum() > 5 and ((taps > 0) & (taps < 16)).sum() > 20      # each tap's compare, both ways
    for k in ("dot_negative", "min_is_shadow", "floor_taken"):                         # the selections, both ways
        assert 0 < counts[k] < cov.sum(), k
    assert (~r["early"] & cov).sum() > 100


def test_fp32_fragment_stage_against_float64(passes):
    """two conditions on the scene: at most 2 % of the covered pixels undecided, and the fp32 restatement within 1e-4 relative on every decided one"""
    r32, r64 = passes["r32"], passes["r64"]
    cov, und = r64["covered"], ref.undecided(r64)
    assert und.sum() <= ref.MAX_UNDECIDED_FRACTION * cov.sum(), (int(und.sum()), int(cov.sum()))
    ok = ref.within(r32["main"], r64["main"]).all(-1)
    assert ok[cov & ~und].all(), np.argwhere(cov & ~und & ~ok)[:5].tolist()
    allowed = ref.within(r32["main"][None], ref.allowed_outcomes(r64)).all(-1).any(0)
    assert allowed[und].all()
    assert (r32["main"][~cov] == passes["scene"]["main0"][~cov]).all()
    # the receivers sit far behind their occluders: no decided tap is nearer than the bias to its threshold
    assert r64["tap_margin"][cov & ~r64["early"] & ~und].min() > 5e-6


def _header_struct(name):
    text = (ROOT / "include" / "sailor_hip.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    return [int(v) for v in re.findall(r"/\*\s*(\d+) \*/", body)]


def test_structs_and_symbols():
    assert C.sizeof(_lib.ParticleData) == 80 and C.sizeof(_lib.ParticleInstance) == 112 and C.sizeof(_lib.ParticlesConstants) == 20
    assert ref.RECORD_DTYPE.itemsize == 80 and ref.INSTANCE_DTYPE.itemsize == 112
    off = lambda s, names: [getattr(s, n).offset for n in names]
    assert _header_struct("SailorParticleData") == off(_lib.ParticleData, ["enabled", "xyz1", "rgba1", "xyz2", "rgba2"]) == [0, 16, 32, 48, 64]
    assert _header_struct("SailorParticleInstance") == off(_lib.ParticleInstance, ["model", "color", "colorOld", "materialInstance", "isCulled", "_pad"]) == [0, 64, 80, 96, 100, 104]
    assert _header_struct("SailorParticlesConstants") == off(_lib.ParticlesConstants, ["numInstances", "numFrames", "fps", "traceFrames", "traceDecay"]) == [0, 4, 8, 12, 16]
    assert [ref.INSTANCE_DTYPE.fields[n][1] for n in ("model", "color", "colorOld", "materialInstance", "isCulled", "_pad")] == [0, 64, 80, 96, 100, 104]
    lib = _lib.load()
    for name in ("sailor_hip_particles_update", "sailor_hip_particles_workspace_bytes", "sailor_hip_particles_shadow", "sailor_hip_particles_draw"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.sailor_hip_particles_workspace_bytes(48, 80, 72, 40) == 8 * 48 * 80 and lib.sailor_hip_particles_workspace_bytes(0, 80, 72, 40) == 0
    assert lib.sailor_hip_particles_workspace_bytes(48, 80, 72, 32769) == 0 and lib.sailor_hip_particles_workspace_bytes(5, 3, 7, 9) == 512


def test_the_host_mirror_and_the_fixture():
    from sailor_amd.runtime_binding import load
    rt = load()
    assert rt.sailor_rt_node_registered(b"ExperimentalParticles") == 0          # an opt-in class, like Bloom, Clear and ShadowPrepass
    assert rt.sailor_rt_enable_node(None, b"ExperimentalParticles") == -1       # no runtime to opt in
    assert hasattr(rt, "sailor_rt_set_particles")
    text = (ROOT / "tests" / "golden" / "ExperimentalRenderer.renderer").read_text()
    entries = re.findall(r"^- name: (\w+)", text[text.index("\nframe:"):], re.M)
    # (the shipped file lists ten frame entries)
    assert entries == ["Clear", "Clear", "LinearizeDepth", "DebugDraw", "LightCulling", "ShadowPrepass", "Sky", "ExperimentalParticles", "PostProcess", "RenderImGui"]
    inst = host.particle_instances(cases.pass_scene()["records"][7:], 7, 1, material_instance=3)
    assert (inst["color"] == 1).all() and (inst["colorOld"] == 0).all() and inst["model"][0].tolist() == [f32(2 / 3), 0, 0, 0, 0, f32(2 / 3), 0, 0, 0, 0, f32(2 / 3), 0, -4, 2, -14, 1]
