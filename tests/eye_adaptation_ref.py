"""Two independent NumPy restatements of the EyeAdaptation node's three passes (FrameGraph/EyeAdaptationNode.cpp:22-221;
Content/Shaders/ComputeHistogram.shader, ComputeAverageLuminance.shader, Tonemapping.shader, Formats.glsl:1-51).

  * `Ref32`: float32 throughout, one rounding per written operation, the evaluation order include/sailor_hip.h fixes
    (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; mat3 * v row by row; vec3 / float = three divisions; fp32 literals) and the
    same fixed log2 / exp2 algorithms as sailor_amd/csrc/eye_adaptation.hip.  The kernels are compared with it bit for bit.
  * `Ref64`: float64 with np.log2 / np.exp2: what the shaders mean.  Ref32 is compared with it under tolerances.

Both take the image as (H, W, 4) and keep the reference's quirks: only x < 16 (W // 16), y < 16 (H // 16) are counted, numPixels is W H,
the weighted sum is uint32 and wraps, a black pixel under LUMINANCE is NaN.  Defined where GLSL is not: NaN luminance -> bin 0, +inf -> bin 255.
"""
import numpy as np

ACES, UNCHARTED2, LUMINANCE = 1, 2, 4
OPERATOR_SETS = (0, ACES, UNCHARTED2, LUMINANCE, ACES | LUMINANCE, UNCHARTED2 | LUMINANCE)  # the six distinct bodies (ACES wins over UNCHARTED2)
MIN_LOG2, MAX_LOG2, EYE_REACTION = -8.0, 4.0, 3.6  # EyeAdaptationNode.cpp:154-156

f32 = np.float32


def canonical_log2f(x):
    """fixed fp32 log2 of finite x >= 2^-126 (Cephes' single-precision form), as in eye_adaptation.hip"""
    x = np.asarray(x, f32)
    u = x.view(np.uint32)
    e = (u >> np.uint32(23)).astype(np.int32) - np.int32(126)
    m = ((u & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(f32)
    low = m < f32(0.707106781186547524)
    e = np.where(low, e - 1, e)
    m = np.where(low, (m + m) - f32(1.0), m - f32(1.0)).astype(f32)
    z = m * m
    p = np.full_like(m, f32(7.0376836292e-2))
    for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1,
              3.3333331174e-1):
        p = p * m + f32(c)
    y = m * (z * p)
    y = y - f32(0.5) * z
    k = f32(0.44269504088896340736)
    r = y * k
    r = r + m * k
    r = r + y
    r = r + m
    return (r + e.astype(f32)).astype(f32)


def canonical_exp2f(x):
    """fixed fp32 exp2, argument clamped to [-126, 127]; NaN in, NaN out"""
    x0 = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        x = np.where(x0 > f32(127.0), f32(127.0), x0).astype(f32)
        x = np.where(x < f32(-126.0), f32(-126.0), x).astype(f32)
        n = np.floor(x)
        r = x - n
        up = r > f32(0.5)
        n = np.where(up, n + f32(1.0), n).astype(f32)
        r = np.where(up, r - f32(1.0), r).astype(f32)
        p = np.full_like(r, f32(1.535336188319500e-4))
        for c in (1.339887440266574e-3, 9.618437357674640e-3, 5.550332471162809e-2, 2.402264791363012e-1, 6.931472028550421e-1):
            p = p * r + f32(c)
        y = p * r + f32(1.0)
        out = np.ldexp(y, np.where(np.isnan(n), 0, n).astype(np.int32)).astype(f32)
    return np.where(np.isnan(x0), x0, out).astype(f32)


def counted_region(image):
    """EyeAdaptationNode.cpp:173-174: extent / 16 groups by integer division"""
    h, w = image.shape[:2]
    return image[: h // 16 * 16, : w // 16 * 16]


def weighted_sum_u32(counts):
    """ComputeAverageLuminance.shader:43-59 in uint32: products and sum wrap"""
    c = np.asarray(counts).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return np.uint32(int((c * np.arange(256, dtype=np.uint64)).sum()) & 0xFFFFFFFF)


class Ref32:
    dtype = f32

    @staticmethod
    def constants(width, height, delta_time):
        """(minLog2, invRange, range, numPixels, timeCoeff), EyeAdaptationNode.cpp:154-170 (timeCoeff through a float64 exp2 rounded once:
        within an ulp of any exp2f)"""
        rng = f32(MAX_LOG2) - f32(MIN_LOG2)
        t = f32(1.0) - f32(np.exp2(np.float64(-f32(delta_time) * f32(EYE_REACTION))))
        return f32(MIN_LOG2), f32(1.0) / rng, rng, f32(width) * f32(height), f32(min(max(t, f32(0.0)), f32(1.0)))

    @staticmethod
    def bins(rgb, min_log=f32(MIN_LOG2), inv_range=f32(1.0) / f32(12.0)):
        rgb = np.asarray(rgb, f32)
        with np.errstate(all="ignore"):
            lum = (rgb[..., 0] * f32(0.2125) + rgb[..., 1] * f32(0.7154)) + rgb[..., 2] * f32(0.0721)
            lit = lum >= f32(0.005)  # False for NaN
            inf = lum == f32(np.inf)
            safe = np.where(lit & ~inf, lum, f32(1.0)).astype(f32)
            t = (canonical_log2f(safe) - f32(min_log)) * f32(inv_range)
            t = np.where(t < f32(0.0), f32(0.0), np.where(t > f32(1.0), f32(1.0), t)).astype(f32)
            f = t * f32(254.0) + f32(1.0)
            b = np.where(f < f32(256.0), f, f32(255.0)).astype(np.uint32)
        return np.where(lit, np.where(inf, np.uint32(255), b), np.uint32(0)).astype(np.uint32)

    @classmethod
    def histogram(cls, image, min_log=f32(MIN_LOG2), inv_range=f32(1.0) / f32(12.0)):
        b = cls.bins(counted_region(np.asarray(image)[..., :3]), min_log, inv_range)
        return np.bincount(b.reshape(-1), minlength=256).astype(np.uint32)

    @staticmethod
    def average(counts, last, min_log, log_range, num_pixels, time_coeff):
        s = f32(weighted_sum_u32(counts))
        lit = f32(num_pixels) - f32(np.uint32(counts[0]))
        with np.errstate(all="ignore"):
            wla = s / (lit if lit > f32(1.0) else f32(1.0)) - f32(1.0)
            lum = canonical_exp2f(((wla / f32(254.0)) * f32(log_range)) + f32(min_log))[()]
            last = f32(last)
            return f32(last + (lum - last) * f32(time_coeff))

    @staticmethod
    def _dot(a, v):
        return (f32(a[0]) * v[0] + f32(a[1]) * v[1]) + f32(a[2]) * v[2]

    @staticmethod
    def _partial(x):
        A, B, C_, D, E, F = f32(0.15), f32(0.50), f32(0.10), f32(0.20), f32(0.02), f32(0.30)
        return ((x * (A * x + C_ * B) + D * E) / (x * (A * x + B) + D * F)) - E / F

    @classmethod
    def tonemap(cls, image, avg, ops, white_point=(1.4, 1.5, 1.4), exposure=1.0):
        return _tonemap(cls, f32, image, avg, ops, white_point, exposure)


class Ref64:
    dtype = np.float64

    @staticmethod
    def constants(width, height, delta_time):
        rng = MAX_LOG2 - MIN_LOG2
        t = 1.0 - np.exp2(-float(delta_time) * EYE_REACTION)
        return MIN_LOG2, 1.0 / rng, rng, float(width) * float(height), min(max(t, 0.0), 1.0)

    @staticmethod
    def bins(rgb, min_log=MIN_LOG2, inv_range=1.0 / 12.0):
        rgb = np.asarray(rgb, np.float64)
        with np.errstate(all="ignore"):
            lum = rgb @ np.array([np.float64(f32(0.2125)), np.float64(f32(0.7154)), np.float64(f32(0.0721))])
            lit = lum >= np.float64(f32(0.005))
            inf = lum == np.inf
            t = np.clip((np.log2(np.where(lit & ~inf, lum, 1.0)) - min_log) * inv_range, 0.0, 1.0)
            b = (t * 254.0 + 1.0).astype(np.uint32)
        return np.where(lit, np.where(inf, np.uint32(255), b), np.uint32(0)).astype(np.uint32)

    @classmethod
    def histogram(cls, image, min_log=MIN_LOG2, inv_range=1.0 / 12.0):
        b = cls.bins(counted_region(np.asarray(image)[..., :3]), min_log, inv_range)
        return np.bincount(b.reshape(-1), minlength=256).astype(np.uint32)

    @staticmethod
    def average(counts, last, min_log, log_range, num_pixels, time_coeff):
        s = float(weighted_sum_u32(counts))
        wla = s / max(float(num_pixels) - float(counts[0]), 1.0) - 1.0
        lum = float(np.exp2(wla / 254.0 * float(log_range) + float(min_log)))
        return float(last) + (lum - float(last)) * float(time_coeff)

    @staticmethod
    def _dot(a, v):
        return np.float64(f32(a[0])) * v[0] + np.float64(f32(a[1])) * v[1] + np.float64(f32(a[2])) * v[2]

    @staticmethod
    def _partial(x):
        A, B, C_, D, E, F = (np.float64(f32(v)) for v in (0.15, 0.50, 0.10, 0.20, 0.02, 0.30))
        return ((x * (A * x + C_ * B) + D * E) / (x * (A * x + B) + D * F)) - E / F

    @classmethod
    def tonemap(cls, image, avg, ops, white_point=(1.4, 1.5, 1.4), exposure=1.0):
        return _tonemap(cls, np.float64, image, avg, ops, white_point, exposure)


# Tonemapping.shader:76-87 (column-major constructors: these are the ROWS of the matrices) and Formats.glsl:7-9, 30-32
_ACES_IN = ((0.59719, 0.35458, 0.04823), (0.07600, 0.90834, 0.01566), (0.02840, 0.13383, 0.83777))
_ACES_OUT = ((1.60475, -0.53108, -0.07367), (-0.10208, 1.10813, -0.00605), (-0.00327, -0.07276, 1.07602))
_RGB2XYZ = ((0.4124564, 0.3575761, 0.1804375), (0.2126729, 0.7151522, 0.0721750), (0.0193339, 0.1191920, 0.9503041))
_XYZ2RGB = ((3.2404542, -1.5371385, -0.4985314), (-0.9692660, 1.8760108, 0.0415560), (0.0556434, -0.2040259, 1.0572252))


def _tonemap(R, T, image, avg, ops, white_point, exposure):
    """Tonemapping.shader:135-161 in the number type T (literals are their fp32 values in both)"""
    lit = lambda v: T(f32(v))
    image = np.asarray(image, f32)
    px = [image[..., c].astype(T) for c in range(3)]
    aces, lum = bool(ops & ACES), bool(ops & LUMINANCE)
    u2 = bool(ops & UNCHARTED2) and not aces
    with np.errstate(all="ignore"):
        scale = lit(9.6) * T(f32(avg)) + lit(0.0001)
        if lum:
            X, Y, Z = (R._dot(row, px) for row in _RGB2XYZ)
            inv = T(1.0) / ((X + Y) + Z)
            Yx, Yy = X * inv, Y * inv
            c = [Y / scale] * 3
        else:
            c = [p / scale for p in px]
        if aces:
            v = [R._dot(row, c) for row in _ACES_IN]
            v = [(x * (x + lit(0.0245786)) - lit(0.000090537)) / (x * (lit(0.983729) * x + lit(0.4329510)) + lit(0.238081)) for x in v]
            c = [R._dot(row, v) for row in _ACES_OUT]
            c = [np.where(x < 0, T(0.0), np.where(x > 1, T(1.0), x)).astype(T) for x in c]
        elif u2:
            ws = [T(1.0) / R._partial(T(f32(w))) for w in white_point[:3]]
            c = [R._partial(x * T(f32(exposure))) * w for x, w in zip(c, ws)]
        if lum:
            xyz = [c[0] * Yx / Yy, c[0], c[0] * ((T(1.0) - Yx) - Yy) / Yy]
            c = [R._dot(row, xyz) for row in _XYZ2RGB]
        out = np.empty(image.shape, T)
        for k in range(3):
            out[..., k] = c[k]
        out[..., 3] = image[..., 3]
    return out


def step(R, image, last, delta_time, ops, white_point=(1.4, 1.5, 1.4), exposure=1.0, constants=None):
    """the node's sequence for one frame: (counts, adapted luminance, LDR image); `constants` = the five push constants if not R's own"""
    h, w = image.shape[:2]
    min_log, inv_range, log_range, num_pixels, time_coeff = constants or R.constants(w, h, delta_time)
    counts = R.histogram(image, min_log, inv_range)
    lum = R.average(counts, last, min_log, log_range, num_pixels, time_coeff)
    return counts, lum, R.tonemap(image, lum, ops, white_point, exposure)


def same_bits_or_class(a, b):
    """float32 arrays equal bit for bit where finite; non-finite values by class (NaN / +inf / -inf), as tests/test_shade_gpu.py compares them"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    fin = np.isfinite(a) & np.isfinite(b)
    ok = np.where(fin, a.view(np.uint32) == b.view(np.uint32),
                  (np.isnan(a) & np.isnan(b)) | (np.isposinf(a) & np.isposinf(b)) | (np.isneginf(a) & np.isneginf(b)))
    return ok
