"""Two NumPy restatements of the sky kernels (sailor_amd/csrc/sky.hip = Content/Shaders/Sky.shader under {FILL}, {}, {SUN}, {COMPOSE}).

Ref32 is the specification of the kernels: every intermediate is np.float32, every operation is one IEEE rounding in the order sky.hip writes it,
exp is the fixed fp32 algorithm of canonical_math.h, the small sines and cosines of Rotate are the kernel's polynomials, and the sums run in the
shader's sequential order.  Ref64 is the literal shader in float64 with np.exp / np.sin / np.cos / pow and atan2; its only job is to show that Ref32
has no transcription error.  Both take the matrices the kernels take (view, invProjection as float32[16], column-major) and the inverse of the view
the library's host code hands the kernel, so that what is compared is the shader and not a matrix inversion.

Images are (h, w, 4) arrays, row 0 = top; texel (i, j) has the quad's inTexcoord ((i + 0.5) / w, (j + 0.5) / h); alpha is 0.
"""
import math

import numpy as np

from eye_adaptation_ref import canonical_exp2f

f32 = np.float32
R = 6371000.0
ATMOSPHERE_R = 160000.0
SUN_ANGULAR_R = math.radians(0.545)
PI = 3.14159265359
B0R = (3.8e-6, 13.5e-6, 33.1e-6)
B0MIE = 22e-6
H0R, H0MIE = 7994.0, 1200.0
STEPS = 127
SKY_RESOLUTION, SUN_RESOLUTION, ENV_CUBEMAP_SIZE, ENV_CUBEMAP_LEVELS = 256, 32, 256, 8   # SkyNode.h:13-15, SkyNode.cpp:755

PARAM_DEFAULTS = dict(cloudsAttenuation1=0.3, cloudsAttenuation2=0.06, cloudsDensity=0.3, cloudsCoverage=0.56, phaseInfluence1=0.025, phaseInfluence2=0.9,
                      eccentrisy1=0.95, eccentrisy2=0.51, fog=10.0, sunIntensity=500.0, ambient=0.5, scatteringSteps=5, scatteringDensity=0.5,
                      scatteringIntensity=0.5, scatteringPhase=0.5, sunShaftsIntensity=0.45, sunShaftsDistance=60)   # SkyNode.h:51-67
PARAM_OFFSETS = dict(lightDirection=0, **{name: 16 + 4 * k for k, name in enumerate(PARAM_DEFAULTS)})                # Sky.shader:116-136, std140


class _Ref:
    F = None

    # ---- primitives the two restatements differ in --------------------------------------------------------------------------------------------
    def exp(self, x):
        raise NotImplementedError

    def pow15(self, v):
        raise NotImplementedError

    def sincos_small(self, x):
        raise NotImplementedError

    def facing_sun(self, dirv, sun, up):
        raise NotImplementedError

    # ---- shared vocabulary --------------------------------------------------------------------------------------------------------------------
    def c(self, x):
        return self.F(x)

    def arr(self, x):
        return np.asarray(x, self.F)

    def dot(self, a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def length(self, a):
        return np.sqrt(self.dot(a, a))

    def sub(self, a, b):
        return (a[0] - b[0], a[1] - b[1], a[2] - b[2])

    def madd(self, a, d, t):
        return (a[0] + d[0] * t, a[1] + d[1] * t, a[2] + d[2] * t)

    def normalize(self, a):
        l = self.length(a)
        return (a[0] / l, a[1] / l, a[2] / l)

    def cross(self, a, b):
        return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])

    def mul(self, M, x, y, z, w):
        """GLSL mat4 * vec4, M column-major: ((c0 x + c1 y) + c2 z) + c3 w per row"""
        return tuple(((M[r] * x + M[4 + r] * y) + M[8 + r] * z) + M[12 + r] * w for r in range(4))

    def where3(self, m, a, b):
        return tuple(np.where(m, x, y) for x, y in zip(a, b))

    def ray_sphere(self, r0, rd, sr):   # Math.glsl:242-264, s0 = 0, a = 1
        c_ = self.c
        b = c_(2.0) * self.dot(rd, r0)
        c = self.dot(r0, r0) - c_(sr) * c_(sr)
        disc = b * b - c_(4.0) * c
        miss = disc < 0
        tmp = np.sqrt(np.where(miss, c_(0.0), disc))
        x1, x2 = (-b + tmp) / c_(2.0), (-b - tmp) / c_(2.0)
        lo, hi = np.where(x1 < x2, x1, x2), np.where(x1 < x2, x2, x1)
        return np.where(miss, c_(-1.0), lo), np.where(miss, c_(-1.0), hi)

    def intersect_sphere(self, origin, direction, earth):   # Sky.shader:218-245
        c_ = self.c
        ix, iy = self.ray_sphere(origin, direction, R + ATMOSPHERE_R)
        outer = np.where(ix < 0, iy, ix)
        shift = np.where(outer < c_(ATMOSPHERE_R * 10), outer, c_(ATMOSPHERE_R * 10))
        if earth:
            tx, ty = self.ray_sphere(origin, direction, R)
            inner = np.where(tx > 0, tx, ty)
            shift = np.where(inner > 0, inner * c_(3.0), shift)
        hit = self.madd(origin, direction, shift)
        return self.where3(outer <= 0, tuple(np.broadcast_to(o, np.shape(outer)) for o in origin), hit)

    def uniforms(self, view, inv_projection, inv_view, camera_position, light_direction):
        c_ = self.c
        cam = [c_(f32(x)) for x in camera_position[:3]]
        l = [c_(f32(x)) for x in light_direction[:3]]
        u = dict(invProjection=self.arr(np.asarray(inv_projection, f32)), invView=self.arr(inv_view), view=self.arr(np.asarray(view, f32)))
        u["origin"] = (c_(0.0) + cam[0] * c_(0.01), c_(R) + cam[1] * c_(0.01), c_(0.0) + cam[2] * c_(0.01))   # :610
        u["sun"] = self.normalize((-l[0], -l[1], -l[2]))                                                     # :611
        u["right"] = self.normalize(self.cross(u["sun"], (c_(0.0), c_(1.0), c_(0.0))))                         # :623
        u["up"] = self.cross(u["right"], u["sun"])
        u["axis2"] = self.cross(u["sun"], u["up"])                                                             # :703
        return u

    def texcoords(self, w, h, rows=None):
        c_ = self.c
        j0, j1 = (0, h) if rows is None else rows
        i, j = np.meshgrid(np.arange(w), np.arange(j0, j1))
        u = (i.astype(self.F) + c_(0.5)) / c_(w)
        v = (j.astype(self.F) + c_(0.5)) / c_(h)
        return u, v

    def view_direction(self, U, tx, ty):   # :729-731, :617-619
        c_ = self.c
        v = self.mul(U["invProjection"], tx * c_(2.0) - c_(1.0), ty * c_(2.0) - c_(1.0), c_(1.0), c_(1.0))
        w = self.mul(U["invView"], v[0] / v[3], v[1] / v[3], v[2] / v[3], c_(0.0))
        l = np.sqrt(((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]) + w[3] * w[3])
        return (w[0] / l, w[1] / l, w[2] / l)

    def phase_mie(self, x):   # :193-199
        c_ = self.c
        q = []
        for cc, dd, ee in zip((.256098, .132268, .010016), (-1.5, -1.74, -1.98), (1.5625, 1.7569, 1.9801)):
            den = c_(dd) * x + c_(ee)
            q.append(((x * x + c_(1.0)) * c_(cc)) / self.pow15(den))
        t = c_(.33333333333)
        return (q[0] * t + q[1] * t) + q[2] * t

    def sky_lighting(self, origin, direction, sun, earth):   # :277-379 without SUN
        c_ = self.c
        n = np.shape(direction[0])
        origin = tuple(np.broadcast_to(o, n) for o in origin)
        destination = self.intersect_sphere(origin, direction, earth)
        d = self.sub(destination, origin)
        dl = self.length(d)
        dead = dl < c_(0.01)
        safe = np.where(dead, c_(1.0), dl)
        angle = self.dot((d[0] / safe, d[1] / safe, d[2] / safe), sun)
        step = (d[0] / c_(128.0), d[1] / c_(128.0), d[2] / c_(128.0))
        d_step = self.length(step)
        res_r = [np.zeros(n, self.F) for _ in range(3)]
        res_m = [np.zeros(n, self.F) for _ in range(3)]
        density_r, density_m = np.zeros(n, self.F), np.zeros(n, self.F)
        log_mie11 = c_(B0MIE) * c_(1.1)
        with np.errstate(over="ignore", invalid="ignore"):
            for i in range(STEPS):
                point = self.madd(origin, step, c_(i + 1))
                h = self.length(point) - c_(R)
                hr = self.exp(-h / c_(H0R)) * d_step
                hm = self.exp(-h / c_(H0MIE)) * d_step
                density_r = density_r + hr
                density_m = density_m + hm
                to_light = self.intersect_sphere(point, tuple(np.broadcast_to(s, n) for s in sun), earth)
                h_light = self.length(to_light) - c_(R)
                step_to_light = (h_light - h) / c_(8.0)
                d_step_light = self.length(self.sub(to_light, point)) / c_(8.0)
                light_r, light_m = np.zeros(n, self.F), np.zeros(n, self.F)
                reached = np.ones(n, bool)
                for j in range(8):
                    h1 = h + step_to_light * c_(j)
                    reached &= ~(h1 < 0)
                    light_m = light_m + self.exp(-h1 / c_(H0MIE)) * d_step_light
                    light_r = light_r + self.exp(-h1 / c_(H0R)) * d_step_light
                sum_r, sum_m = density_r + light_r, light_m + density_m
                for k in range(3):
                    aggr = self.exp(-c_(B0R[k]) * sum_r - log_mie11 * sum_m)
                    res_r[k] = np.where(reached, res_r[k] + aggr * hr, res_r[k])
                    res_m[k] = np.where(reached, res_m[k] + aggr * hm, res_m[k])
            phase_r = ((c_(3.0) * c_(PI)) / c_(16.0)) * (c_(1.0) + angle * angle)
            phase_m = self.phase_mie(angle)
            out = [c_(7.0) * ((c_(B0R[k]) * res_r[k]) * phase_r + (c_(B0MIE) * res_m[k]) * phase_m) for k in range(3)]
        return [np.where(dead, c_(0.0), o) for o in out]

    def _image(self, rgb, h, w):
        out = np.zeros((h, w, 4), self.F)
        for k in range(3):
            out[..., k] = rgb[k].reshape(h, w)
        return out

    # ---- the four define sets -----------------------------------------------------------------------------------------------------------------
    def fill(self, U, w, h):
        """{FILL}: SkyLighting with the Earth test"""
        u, v = self.texcoords(w, h)
        direction = self.view_direction(U, u.ravel(), (self.c(1.0) - v).ravel())
        return self._image(self.sky_lighting(U["origin"], direction, U["sun"], True), h, w)

    def env_face(self, U, size):
        """{}: the same without the Earth test; U carries the face's matrices"""
        u, v = self.texcoords(size, size)
        direction = self.view_direction(U, u.ravel(), (self.c(1.0) - v).ravel())
        return self._image(self.sky_lighting(U["origin"], direction, U["sun"], False), size, size)

    def quat_mult(self, a, b):   # Math.glsl:47-55, (x, y, z, w)
        return ((((a[3] * b[0]) + (a[0] * b[3])) + (a[1] * b[2])) - (a[2] * b[1]),
                (((a[3] * b[1]) - (a[0] * b[2])) + (a[1] * b[3])) + (a[2] * b[0]),
                (((a[3] * b[2]) + (a[0] * b[1])) - (a[1] * b[0])) + (a[2] * b[3]),
                (((a[3] * b[3]) - (a[0] * b[0])) - (a[1] * b[1])) - (a[2] * b[2]))

    def rotate(self, v, axis, angle):   # Math.glsl:30-40, :57-74
        s, c = self.sincos_small(angle / self.c(2.0))
        q = (axis[0] * s, axis[1] * s, axis[2] * s, c)
        conj = (-q[0], -q[1], -q[2], q[3])
        zero = np.zeros_like(s)
        r = self.quat_mult(self.quat_mult(q, (v[0] + zero, v[1] + zero, v[2] + zero, zero)), conj)
        return (r[0], r[1], r[2])

    def sun(self, U, w, h):
        """{SUN} with the cleared clouds target"""
        c_ = self.c
        S, zeta = c_(SUN_ANGULAR_R), c_(math.cos(SUN_ANGULAR_R))
        u, v = self.texcoords(w, h)
        tx, ty = u.ravel(), (c_(1.0) - v).ravel()
        ax = -S * (c_(1.0) - tx) + S * tx
        ay = -S * (c_(1.0) - ty) + S * ty
        view_dir = self.rotate(U["sun"], U["up"], ax)
        direction = self.normalize(self.rotate(view_dir, U["axis2"], ay))
        n = tx.shape
        origin = tuple(np.broadcast_to(o, n) for o in U["origin"])
        destination = self.intersect_sphere(origin, direction, False)
        dead = self.length(self.sub(destination, origin)) < c_(0.01)
        theta = self.dot(direction, U["sun"])
        ex, ey = self.ray_sphere(origin, direction, R)
        clear = np.where(ex < ey, ey, ex) < 0
        q = (c_(1.0) - theta) / (c_(1.0) - zeta)
        t = c_(1.0) - self.sq(q)
        attenuation = c_(0.83) * (c_(1.0) - t) + c_(1.0) * t
        value = (attenuation * c_(1.0)) * c_(12000000.0)
        value = np.where(dead | (theta < zeta) | ~clear, c_(0.0), value)
        return self._image([value, value, value], h, w)

    def sq(self, x):
        return x * x

    def _bilinear(self, tex, u, v, repeat):
        c_ = self.c
        H, W = tex.shape[:2]
        x, y = u * c_(W) - c_(0.5), v * c_(H) - c_(0.5)
        fx, fy = np.floor(x), np.floor(y)
        ax, ay = (x - fx)[..., None], (y - fy)[..., None]
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        if repeat:
            x0, y0 = x0 % W, y0 % H
            x1, y1 = (x0 + 1) % W, (y0 + 1) % H
        else:
            x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
            x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
        t = tex[..., :3]
        one = c_(1.0)
        top = t[y0, x0] * (one - ax) + t[y0, x1] * ax
        bot = t[y1, x0] * (one - ax) + t[y1, x1] * ax
        return top * (one - ay) + bot * ay

    def compose(self, U, sky, sun, w, h, rows=None):
        """{COMPOSE} over framebuffer rows [rows[0], rows[1]) (default: all)"""
        c_ = self.c
        S = c_(SUN_ANGULAR_R)
        sky, sun = self.arr(sky), self.arr(sun)
        u, v = self.texcoords(w, h, rows)
        direction = self.view_direction(U, u, c_(1.0) - v)
        out = self._bilinear(sky, u, v, True)
        rel = self.sub(direction, U["sun"])
        dx, dy = self.dot(rel, U["right"]), self.dot(rel, U["up"])
        inside = (dx > -S) & (dy > -S) & (dx < S) & (dy < S) & self.facing_sun(direction, U["sun"], U["up"])
        su = c_(1.0) - (dx / S + c_(1.0)) / c_(2.0)
        sv = c_(1.0) - (dy / S + c_(1.0)) / c_(2.0)
        s = self._bilinear(sun, np.where(inside, su, c_(0.5)), np.where(inside, sv, c_(0.5)), False)
        lum = (s[..., 0] * s[..., 0] + s[..., 1] * s[..., 1]) + s[..., 2] * s[..., 2]
        t = np.where(lum < c_(1.0), lum, c_(1.0))[..., None]   # clamp(0, 1, luminance) = min(max(0, 1), luminance)
        with np.errstate(invalid="ignore"):
            m = out * (c_(1.0) - t) + s * t
            merged = np.where(out < m, m, out)
        res = np.zeros(out.shape[:2] + (4,), self.F)
        res[..., :3] = np.where(inside[..., None], merged, out)
        return res


class Ref32(_Ref):
    F = f32

    def exp(self, x):
        return canonical_exp2f(x * f32(1.442695))

    def pow15(self, v):
        return v * np.sqrt(v)

    def sincos_small(self, x):
        x2 = x * x
        s = x * (f32(1.0) + x2 * (f32(-0.16666667) + x2 * f32(0.008333334)))
        c = f32(1.0) + x2 * (f32(-0.5) + x2 * f32(0.041666668))
        return s, c

    def facing_sun(self, dirv, sun, up):
        return self.dot(dirv, sun) > 0


class Ref64(_Ref):
    F = np.float64

    def exp(self, x):
        return np.exp(x)

    def pow15(self, v):
        return np.power(v, 1.5)

    def sq(self, x):
        return np.power(x, 2.0)

    def sincos_small(self, x):
        return np.sin(x), np.cos(x)

    def facing_sun(self, dirv, sun, up):   # Sky.shader:629, :635
        n = np.shape(dirv[0])
        angle = np.arctan2(self.dot(self.cross(dirv, tuple(np.broadcast_to(s, n) for s in sun)), up), self.dot(dirv, sun))
        return np.abs(angle) < PI * 0.5


def uniforms_from_frame(ref, frame, inv_view, light_direction):
    """the uniforms of FILL / SUN / COMPOSE from a _lib.UboFrameData"""
    return ref.uniforms(list(frame.view), list(frame.invProjection), inv_view, list(frame.cameraPosition), light_direction)


def inv_view_for(ref, view):
    """Ref32 takes the inverse the library's host code computes; Ref64 inverts the float32 view in float64"""
    if ref.F is f32:
        from sailor_amd import host
        return host.mat4_inverse(np.asarray(view, f32))
    return np.linalg.inv(np.asarray(view, np.float64).reshape(4, 4).T).T.reshape(-1)


def chain_offsets(size, levels):
    """float offsets of the levels of the flat RGBA32F cube chain"""
    offs, o = [], 0
    for l in range(levels):
        s = max(size >> l, 1)
        offs.append((o, s))
        o += 6 * s * s * 4
    return offs, o
