"""CPU suite of the clouds path: ABI, the host-side sun colour, the fp32 restatement of tests/clouds_ref.py held against its float64-values twin and against a
literal scalar transliteration of the shader's loops, the coverage every case must have, the blend formula, and the golden plane.  No GPU needed."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import clouds_cases as cc
import clouds_ref as cref
import sky_cases as sc
from eye_adaptation_ref import canonical_exp2f
from sailor_amd import _lib, host

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
R32, R64 = cref.Ref32(), cref.Ref64()
SYMBOLS = ("sailor_hip_sky_clouds", "sailor_hip_sky_sun_clouds", "sailor_hip_sky_blit_clouds", "sailor_host_sky_sun_color")
CAP = 0.005   # the share of a case's texels that may take another exit step in the twin and be left out of the value comparison


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_abi_symbols_version_and_struct_layout():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    declared = set(re.findall(r"\b(sailor_(?:hip|host)_\w+)\s*\(", header))
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in declared and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.sailor_hip_version() >= 7
    assert C.sizeof(_lib.SkyParams) == 84   # every member the march needs was already there


def test_the_plain_sun_still_refuses_a_clouds_plane_in_the_header_too():
    header = (ROOT / "include" / "sailor_hip.h").read_text()
    assert "sailor_hip_sky_sun_clouds takes it" in header


@pytest.mark.parametrize("direction", [(0.0, -1.0, 0.0), (0.0, -1.0, 1.0), (0.2, -1.0, 0.3), (0.0, -0.5, 1.0), (0.0, -0.1, 1.0), (0.3, -0.05, 0.9), (0.0, -0.102, 1.0),
                                       (0.0, -0.0995, 1.0), (0.0, 0.0, 1.0), (0.0, 0.2, 1.0), (1.0, 1.0, 0.0)])
def test_host_sun_color_against_the_restatement(direction):
    """suns above and below border = 0.1 (angle = -direction.y after normalisation), on it, on the horizon and under it"""
    d = np.asarray(direction, f32)
    d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    got, want = host.sky_sun_color(d), np.asarray(R32.sun_color(d), f32)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    wide = np.asarray(R64.sun_color(d))
    assert np.all(np.isfinite(got)) and np.allclose(got, wide, rtol=2e-6, atol=0), (got, wide)
    lib = _lib.load()
    assert lib.sailor_host_sky_sun_color(None, got.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lib.sailor_host_sky_sun_color(d.ctypes.data_as(C.POINTER(C.c_float)), None) == -1


def test_sun_color_end_points():
    assert np.allclose(host.sky_sun_color((0.0, -1.0, 0.0)), (0.925, 0.861, 0.755))            # the zenith
    assert np.allclose(host.sky_sun_color((0.0, 1.0, 0.0)), (0.0998, 0.008, 8.2e-5))           # under the horizon: GroundIlluminance
    assert np.allclose(host.sky_sun_color((0.0, -0.1, 0.0)), (0.6, 0.4490196, 0.1588), atol=1e-6)   # at border both arms meet in HalfIlluminance


def test_textures_are_patchy_and_seeded():
    weather, low, high, noise = cc.textures()
    assert weather.shape == (32, 32, 4) and low.shape == (16, 16, 16) and high.shape == (8, 8, 8) and noise.shape == (16, 16, 4)
    assert weather.dtype == low.dtype == high.dtype == np.uint8 and noise.dtype == f32
    assert low.min() == 0 and low.max() == 255 and high.min() == 0 and high.max() == 255
    assert int(weather[..., 0].astype(np.int64).sum()) == int(cc.textures()[0][..., 0].astype(np.int64).sum())


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_every_case_has_lit_opaque_and_early_texels(name):
    c = cc.case(name)
    _, plane, exit_step = cc.reference(name)
    lit, gone, early = cc.assert_coverage(c, plane, exit_step)
    print(f"{name}: {c.w} x {c.h}, {lit} texels with alpha > 0, {gone} leave on transmittance, {early} return early, exit steps {exit_step.min()} .. {exit_step.max()}")
    assert np.isfinite(plane).all()


def test_cases_cover_the_branches_the_issue_names():
    heights = {c.position[1] for c in cc.CASES}
    assert 150.0 in heights and 1.5e6 in heights and max(heights) > 2.2e6   # under, inside, above the layer (7 .. 22 km)
    assert {0, 2, 5} <= {c.steps for c in cc.CASES} and any(c.time != 0 for c in cc.CASES)
    assert {(c.w, c.h) for c in cc.CASES} == {(24, 16), (72, 10)} and {"far", "wall"} == {c.depth for c in cc.CASES}
    c = cc.case("under_wall_time")
    d = cc.depth_plane(c, cc.make_frame(c))
    assert d[0, 0] == cc.WALL and d[0, -1] == cc.make_frame(c).cameraZNearZFar[1]


# Ref32 against the float64-values twin, measured on the cases of clouds_cases.py (this file prints them; DESIGN.md section 4 carries them):
#   case                        exit steps differ   max |d alpha|   max |d rgb| / plane max
MEASURED_TWIN = {
    "under_up":                   (0, 1.82e-3, 5.10e-4),
    "under_wall_time":            (0, 1.22e-3, 2.37e-4),
    "inside_level":               (0, 1.35e-3, 1.30e-3),
    "inside_wall_one_octave":     (0, 5.40e-4, 4.48e-4),
    "above_down":                 (0, 7.98e-4, 7.61e-4),
    "above_down_no_scattering":   (0, 0.0, 7.76e-8),
    "under_two_octaves_low_sun":  (0, 1.29e-3, 1.00e-3),
}
# The deviation is not rounding noise of the sums: a sample's texture coordinate is shift + position / 9000 of about 709 in fp32 (the height of the layer over
# the Earth's centre, divided by 9000), quantised to 6e-5, i.e. 1e-3 texels of the 16^3 volume, and every density inherits a relative error of that size.
# The bound is 4 x the measured figure of the case itself, per quantity; the all-zero alpha of the case without scattering is held exactly.


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_fp32_restatement_against_the_float64_values_twin(name):
    c = cc.case(name)
    sky, a, ea = cc.reference(name)
    b, eb = cc.run(R64, c, sky=sky)
    differ = ea != eb
    share = differ.mean()
    same = ~differ
    scale = float(np.abs(a[..., :3]).max())
    d_alpha = float(np.abs(a[..., 3] - b[..., 3])[same].max())
    d_rgb = float(np.abs(a[..., :3] - b[..., :3])[same].max()) / scale
    print(f"{name}: exit step differs on {int(differ.sum())} of {differ.size} texels ({share:.4f}), max |d alpha| {d_alpha:.3g}, max |d rgb| / plane max {d_rgb:.3g}")
    assert share <= CAP, (name, int(differ.sum()))
    measured = MEASURED_TWIN[name]
    assert int(differ.sum()) <= 4 * measured[0] and d_alpha <= 4.0 * measured[1] and d_rgb <= 4.0 * measured[2], (name, int(differ.sum()), d_alpha, d_rgb)
    if c.steps == 0:
        assert d_alpha == 0.0
    assert np.array_equal(ea == cref.EARLY, eb == cref.EARLY), "early returns are geometry: the same in both"


def test_design_document_carries_the_measured_twin_figures():
    """DESIGN.md section 4 states the figures this file asserts four times of: one `case` n / alpha / rgb entry per case, in this format"""
    text = (ROOT / "DESIGN.md").read_text()
    for name, (n, a, r) in MEASURED_TWIN.items():
        assert f"`{name}` {n} / {a:.2e} / {r:.2e}" in text, name


# ---- the literal scalar transliteration of Sky.shader:381-595 and :656-692, one texel at a time ----------------------------------------------------
def F(x):
    return f32(x)


def remap(value, lo, hi, new_lo, new_hi):   # :381-384
    return new_lo + (value - lo) / (hi - lo) * (new_hi - new_lo)


def clamp01(x):
    x = x if not x < F(0) else F(0)
    return x if not F(1) < x else F(1)


def vmax(x, y):
    return y if x < y else x


def texel_r8(vol, x, y, z):
    n = vol.shape[0]
    return F(vol[z % n, y % n, x % n]) / F(255)


def fetch3d(vol, u, v, w):
    """trilinear, Repeat: x pairs, then y, then z"""
    n = vol.shape[0]
    c = [t * F(n) - F(0.5) for t in (u, v, w)]
    fl = [np.floor(t) for t in c]
    a = [t - f for t, f in zip(c, fl)]
    x, y, z = (int(f) for f in fl)
    one = F(1)
    plane = []
    for dz in (0, 1):
        top = texel_r8(vol, x, y, z + dz) * (one - a[0]) + texel_r8(vol, x + 1, y, z + dz) * a[0]
        bot = texel_r8(vol, x, y + 1, z + dz) * (one - a[0]) + texel_r8(vol, x + 1, y + 1, z + dz) * a[0]
        plane.append(top * (one - a[1]) + bot * a[1])
    return plane[0] * (one - a[2]) + plane[1] * a[2]


def fetch2d_rgba8(tex, u, v):
    h, w = tex.shape[:2]
    x, y = u * F(w) - F(0.5), v * F(h) - F(0.5)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    xi, yi = int(fx), int(fy)
    t = lambda i, j: tex[j % h, i % w].astype(f32) / F(255)
    one = F(1)
    top = t(xi, yi) * (one - ax) + t(xi + 1, yi) * ax
    bot = t(xi, yi + 1) * (one - ax) + t(xi + 1, yi + 1) * ax
    return top * (one - ay) + bot * ay


def exp32(x):
    return f32(canonical_exp2f(np.asarray(x * F(1.442695), f32)))


def length3(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def ray_sphere(r0, rd, sr):   # Math.glsl:242-264
    b = F(2) * dot3(rd, r0)
    c = dot3(r0, r0) - F(sr) * F(sr)
    disc = b * b - F(4) * c
    if disc < 0:
        return F(-1), F(-1)
    tmp = np.sqrt(disc)
    x1, x2 = (-b + tmp) / F(2), (-b - tmp) / F(2)
    return (x1, x2) if x1 < x2 else (x2, x1)


class Literal:
    def __init__(self, c):
        self.c = c
        self.frame, self.p = cc.make_frame(c), cc.params(c)
        self.U = sc.frame_uniforms(R32.G, self.frame, c.light)
        self.weather, self.low, self.high, self.noise = cc.textures()
        self.time = F(self.frame.currentTime)
        self.sun = [F(x) for x in self.U["sun"]]
        self.origin = [F(x) for x in self.U["origin"]]

    def sample_density(self, position):   # :392-425
        p, t = self.p, self.time
        pos = list(position)
        pos[0] = pos[0] + F(0.1) * t * F(1000)
        pos[2] = pos[2] + F(0.05) * t * F(1000)
        shift1 = [F(-0.0021) * t * F(-0.5), F(0.0017) * t * F(-0.5), F(-0.02) * t * F(-0.5)]
        shift2 = [F(0.021) * t * F(-0.2), F(0.017) * t * F(-0.2), F(0.0) * t * F(-0.2)]
        low = fetch3d(self.low, *[s + q / F(9000) for s, q in zip(shift1, pos)])
        high = fetch3d(self.high, *[s + q / F(1300) for s, q in zip(shift2, pos)])
        weather = fetch2d_rgba8(self.weather, pos[0] / F(409600) + F(0.2), pos[2] / F(409600) + F(0.1))
        start, end = F(cref.CLOUDS_START_R), F(cref.CLOUDS_END_R)
        height = clamp01((abs(pos[1]) - start) / (end - start))
        srb = clamp01(remap(height, F(0), F(0.07), F(0), F(1)))
        srt = clamp01(remap(height, weather[2] * F(0.35), weather[2], F(1), F(0)))
        sa = srb * srt
        drb = height * clamp01(remap(height, F(0), F(0.15), F(0), F(1)))
        drt = height * clamp01(remap(height, F(0.9), F(1), F(1), F(0)))
        da = drb * drt * weather[3] * F(2) * F(p.cloudsDensity)
        sn = low * F(0.85) + high * F(0.15)
        wmc = vmax(weather[0], clamp01(F(p.cloudsCoverage) - F(0.5)) * weather[1] * F(2))
        return clamp01(remap(sn * sa, F(1) - F(p.cloudsCoverage) * wmc, F(1), F(0), F(1))) * da

    def sample_direct_density(self, position):   # :427-448
        avr = (F(cref.CLOUDS_END_R) - F(cref.CLOUDS_START_R)) * F(0.01)
        position, total = list(position), F(0)
        for i in range(4):
            step = avr
            if i == 3:
                step = step * F(6)
            position = [q + s * step for q, s in zip(position, self.sun)]
            total = total + self.sample_density(position) * step
        return total

    def henyey_greenstein(self, a, g):   # :212-216
        g2 = g * g
        v = F(1) + g2 - F(2) * g * a
        return (F(1) - g2) / (F(4) * F(3.1415) * (v * np.sqrt(v)))

    def marching(self, view_dir, max_trace):   # :450-595 -> (colorLow, transmittanceLow, early, exit step)
        p, origin, sun = self.p, self.origin, self.sun
        start, end = cref.CLOUDS_START_R, cref.CLOUDS_END_R
        origin_height = length3(origin)
        s0, s1 = ray_sphere(origin, view_dir, start)
        e0, e1 = ray_sphere(origin, view_dir, end)
        shift_start = vmax(F(0), s1) if s0 < 0 else s0
        inner = vmax(F(0), e1) if e0 < 0 else e0
        shift_end = inner if inner < max_trace else max_trace
        if shift_start > shift_end and e0 < 0:
            return F(0), F(1), True, cref.EARLY
        if origin_height < F(start):
            trace_start = [o + d * shift_start for o, d in zip(origin, view_dir)]
        elif origin_height > F(end):
            trace_start = [o + d * shift_end for o, d in zip(origin, view_dir)]
        else:
            trace_start = list(origin)
        if shift_start > F(cref.BIG_DISTANCE):
            return F(0), F(1), True, cref.EARLY
        mu = vmax(F(0), dot3(view_dir, sun))
        d_a, d_b, d_c = [], [], []
        for j in range(p.scatteringSteps):   # pow(x, j) as the running product
            d_a.append(F(1) if j == 0 else d_a[-1] * F(p.scatteringDensity))
            d_b.append(F(1) if j == 0 else d_b[-1] * F(p.scatteringIntensity))
            d_c.append(F(1) if j == 0 else d_c[-1] * F(p.scatteringPhase))
        position = list(trace_start)
        color_low, trans_low, avr = F(0), F(1), F(150)
        exit_step = cref.RAN_OUT
        for i in range(cref.STEPS):
            density = self.sample_density(position) * avr
            if density > 0:
                for j in range(p.scatteringSteps):
                    random_vec = [F(0), F(0), F(0)]
                    if j > 0:
                        off = F(j) / F(16)
                        nh, nw = self.noise.shape[:2]
                        t = self.noise[int(np.floor((position[2] + off) * F(nh))) % nh, int(np.floor((position[0] + off) * F(nw))) % nw]
                        q = [t[0] - F(0.5), t[1] - F(0.5), t[2] - F(0.5)]
                        l = length3(q)
                        random_vec = [(x / l) * F(10) for x in q]
                    local = [a + b for a, b in zip(position, random_vec)]
                    sun_density = self.sample_direct_density(local)
                    m11 = F(p.phaseInfluence1) * self.henyey_greenstein(mu, d_c[j] * F(p.eccentrisy1))
                    m12 = F(p.phaseInfluence2) * self.henyey_greenstein(mu, d_c[j] * F(p.eccentrisy2))
                    m2 = exp32(-d_a[j] * F(p.cloudsAttenuation1) * sun_density)
                    m3 = F(p.cloudsAttenuation2) * density
                    x0, x1 = ray_sphere(local, sun, cref.R)
                    if vmax(x0, x1) < 0:
                        color_low = color_low + d_b[j] * (m11 + m12) * m2 * m3 * trans_low
                    trans_low = trans_low * exp32(-d_a[j] * F(p.cloudsAttenuation1) * density)
            position = [q + d * avr for q, d in zip(position, view_dir)]
            height = length3(position)
            if trans_low < F(0.05) or height > F(end) or height < F(start) or length3([a - b for a, b in zip(position, trace_start)]) > max_trace:
                exit_step = i
                break
            if i >= 128:
                avr = avr + F(4)
        return color_low, trans_low, False, exit_step

    def texel(self, i, j, sky):   # :656-692
        c, p, G = self.c, self.p, R32.G
        u, v = (F(i) + F(0.5)) / F(c.w), F(1) - (F(j) + F(0.5)) / F(c.h)
        depth = cc.depth_plane(c, self.frame)
        dh, dw = depth.shape
        linear_depth = abs(depth[min(int(np.floor(v * F(dh))), dh - 1), min(int(np.floor(u * F(dw))), dw - 1)])
        d = G.view_direction(self.U, np.asarray([u]), np.asarray([F(1) - v]))
        d = [x[0] for x in d]
        l = length3(d)
        view_dir = [x / l for x in d]
        color = [x for x in R32.bilinear_repeat(np.asarray(sky, f32)[..., :3], np.asarray([u]), np.asarray([v]), lambda t: t)[0]]
        tone = color[2] / (F(1) + color[2])
        horizon = F(1) - exp32(-abs(view_dir[1]) * F(p.fog))
        horizon = horizon * horizon * horizon
        horizon = horizon + (F(1) - clamp01((F(cref.CLOUDS_START_R) - length3(self.origin)) / F(500)))
        horizon = clamp01(horizon)
        z_far = F(self.frame.cameraZNearZFar[1])
        max_trace = F(cref.BIG_DISTANCE) if abs(linear_depth - z_far) < F(1) else linear_depth
        color_low, trans_low, early, exit_step = self.marching(view_dir, max_trace)
        sun_color = [F(x) for x in R32.sun_color([-x for x in self.sun])]
        out = []
        for k in range(3):
            raw = (F(0) if early else F(p.sunIntensity) * sun_color[k] * color_low) + tone * F(p.ambient)
            out.append(color[k] * (F(1) - horizon) + raw * horizon)
        out.append(F(0) if early else F(1) - trans_low)
        return np.asarray(out, f32), exit_step


@pytest.mark.parametrize("name", ["under_up", "inside_level", "above_down", "under_wall_time"])
def test_vectorised_restatement_equals_the_literal_loops(name):
    """a handful of texels per case: one that returns early, one that leaves on transmittance, lit ones that leave the layer, one in each corner region"""
    c = cc.case(name)
    sky, plane, exit_step = cc.reference(name)
    opaque = cc.transmittance_exits(plane, exit_step)
    partial = (plane[..., 3] > 0) & ~opaque
    picks = []
    for mask in (exit_step == cref.EARLY, opaque, partial, partial[::-1, ::-1]):
        at = np.argwhere(mask)
        assert len(at), name
        j, i = at[len(at) // 2]
        if mask is not partial and mask.base is partial:
            j, i = c.h - 1 - j, c.w - 1 - i
        picks.append((int(i), int(j)))
    picks.append((c.w - 1, c.h - 1))
    lit = Literal(c)
    with np.errstate(all="ignore"):
        for i, j in dict.fromkeys(picks):
            got, step = lit.texel(i, j, sky)
            assert step == exit_step[j, i], (name, i, j, step, exit_step[j, i])
            assert np.array_equal(bits(got), bits(plane[j, i])), (name, i, j, got, plane[j, i])


def test_blend_formula_on_hand_made_values():
    src = np.asarray([[1.0, 2.0, 3.0, 0.25], [4.0, 4.0, 4.0, 1.0], [9.0, 9.0, 9.0, 0.0], [2.0, 0.0, 1.0, 0.5]], f32)
    dst = np.asarray([[8.0, 4.0, 0.0, 1.0], [7.0, 7.0, 7.0, 0.5], [1.0, 2.0, 3.0, 0.75], [0.0, 0.0, 0.0, 0.0]], f32)
    want = np.asarray([[0.25 + 6.0, 0.5 + 3.0, 0.75, 0.0625 - 0.75],    # a = src.a^2 - dst.a (1 - src.a): the alpha op is SUBTRACT
                       [4.0, 4.0, 4.0, 1.0],                              # opaque clouds replace the target
                       [1.0, 2.0, 3.0, -0.75],                            # no clouds: the colour stays, the alpha is NEGATED
                       [1.0, 0.0, 0.5, 0.25]], f32)
    assert np.array_equal(R32.blend(src, dst), want)
    assert np.array_equal(R64.blend(src, dst), want.astype(np.float64))
    # the blit samples the clouds plane bilinearly with clamp-to-edge and does not flip y: a 2 x 2 plane over a 4 x 4 target
    clouds = np.zeros((2, 2, 4), f32)
    clouds[0, :, 3] = 1.0
    clouds[0, :, :3] = 5.0
    out = R32.blit(clouds, np.ones((4, 4, 4), f32), 4, 4)
    assert np.all(out[0, :, :3] == 5.0) and np.all(out[3, :, :3] == 1.0) and np.all(out[0, :, 3] == 1.0)
    assert np.array_equal(out[1], np.broadcast_to(np.asarray([0.75 * 5.0 * 0.75 + 0.25, 0.75 * 5.0 * 0.75 + 0.25, 0.75 * 5.0 * 0.75 + 0.25, 0.5625 - 0.25], f32), (4, 4)))
    rows = R32.blit(clouds, np.ones((2, 4, 4), f32), 4, 4, rows=(1, 3))
    assert np.array_equal(rows, out[1:3])


def test_sun_behind_clouds_restatement_on_hand_made_planes():
    c = sc.case("tele_sun")
    frame = sc.make_frame(c.w, c.h, c.position, c.pitch, c.fov)
    U = sc.frame_uniforms(R32.G, frame, c.light)
    pv = cc.proj_view(frame)
    plain = R32.G.sun(U, 16, 16)
    clear, (cu, cv, w) = R32.sun_clouds(U, pv, cc.alpha_plane("zero"), 16, 16)
    assert np.array_equal(bits(clear), bits(plain)) and plain.max() > 0
    assert w.min() > 0 and 0.4 < cu.min() < cu.max() < 0.6 and 0.4 < cv.min() < cv.max() < 0.6   # the sun dead centre of the lens
    opaque = cc.alpha_plane("zero")
    opaque[..., 3] = 0.5
    assert not R32.sun_clouds(U, pv, opaque, 16, 16)[0].any()   # >= 0.5 hides
    opaque[..., 3] = np.nextafter(f32(0.5), f32(0))
    assert np.array_equal(bits(R32.sun_clouds(U, pv, opaque, 16, 16)[0]), bits(plain))
    half, _ = R32.sun_clouds(U, pv, cc.alpha_plane("ramp"), 16, 16)
    assert 0 < (half[..., 0] > 0).sum() < (plain[..., 0] > 0).sum()
    # w = 0: uvView is inf or NaN, the weights are NaN, the alpha is NaN, the texel stays zero
    with np.errstate(all="ignore"):
        assert np.isnan(R32.bilinear_clamp(cc.alpha_plane("ramp"), np.asarray([np.inf, np.nan, -np.inf], f32), np.asarray([0.5, 0.5, np.nan], f32))[..., 3]).all()


def test_golden_plane_of_the_tiny_case():
    gold = np.load(ROOT / "tests" / "golden" / "tiny_clouds.npz")
    c = cc.case(str(gold["case"]))
    sky, plane, exit_step = cc.reference(c.name)
    weather, low, high, noise = cc.textures()
    for key, a in (("weather", weather), ("low", low), ("high", high), ("noise_bits", bits(noise)), ("sky_bits", bits(sky))):
        assert np.array_equal(gold[key], a), key
    assert np.array_equal(gold["clouds_bits"], bits(plane)) and np.array_equal(gold["exit_step"], exit_step)
    assert np.array_equal(gold["sun_color_bits"], bits(host.sky_sun_color(host.sky_params(lightDirection=c.light).lightDirection[:3])))
