"""Two independent NumPy restatements of the HBAO block of the shipped frame graph (tests/golden/DefaultRenderer.renderer:202-264):
the nearest blit (FrameGraph/BlitNode.cpp:88), Content/Shaders/HBAO.shader:81-249 and Content/Shaders/HBAO_Blur.shader:67-111, written from
the shaders' meaning.

  * `Ref32`: float32 throughout, one rounding per written operation, the evaluation order include/sailor_hip.h fixes (dot(a, b) =
    (a.x b.x + a.y b.y) + a.z b.z; mat4 * vec4 row by row left to right; v / s = a division per component; normalize = v / sqrt(dot);
    rcp(x) = 1 / x; mix(a, b, t) = a (1 - t) + b t; products left to right), sinS = x, round = half to even, the canonical exp2 of
    tests/eye_adaptation_ref.py, and the saturating float -> int conversion (NaN -> 0) in the tap computation, spelled with np.where
    because NumPy's own cast gives another value.  The kernels of sailor_amd/csrc/hbao.hip are compared with it bit for bit.
  * `Ref64`: float64, the literal sin(pi / 2 - acos(x)), np.exp2: what the shaders mean.  Ref32 is compared with it by 8-bit codes.

Images are (h, w) planes, row 0 = top; texel (i, j) has fragTexcoord ((i + 0.5) / w, (j + 0.5) / h).  An R8_UNORM target holds what texture()
would return from it: rint(min(max(v, 0), 1) * 255) / 255, NaN -> 0.  `frame` is a _lib.UboFrameData; the noise is (nh, nw, 4) linear texels.
"""
import numpy as np

from eye_adaptation_ref import canonical_exp2f

f32 = np.float32
SHIPPED = dict(occlusionRadius=700.0, occlusionPower=1.5, occlusionAttenuation=0.1, occlusionBias=0.05, noiseScale=25.0)  # .renderer:226-230
SHIPPED_BLUR = dict(sharpness=0.5, distanceScale=2.0, radius=5.0)                                                          # :243-245
DIRECTIONS = ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (-0.7071069, 0.7071068), (0.7071068, 0.7071069), (0.7071069, -0.7071068),
              (-0.7071068, -0.7071069))  # HBAO.shader:69-79


def srgb8_to_linear(texels_u8):
    """the R8G8B8A8_SRGB decode of a sampled texel (TextureAssetInfo.h:31): rgb through the sRGB curve, alpha linear; float32"""
    c = np.asarray(texels_u8, np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    lin[..., 3] = c[..., 3]
    return np.ascontiguousarray(lin.astype(f32))


def blit_indices(src, dst):
    """source index of every destination texel along one axis: the texel containing the destination centre"""
    i = np.arange(dst, dtype=np.int64)
    return ((2 * i + 1) * src) // (2 * dst)


def blit(src, dst_w, dst_h):
    src = np.asarray(src)
    return np.ascontiguousarray(src[np.ix_(blit_indices(src.shape[0], dst_h), blit_indices(src.shape[1], dst_w))])


def codes(plane):
    """the 8-bit codes an R8_UNORM plane holds"""
    return np.rint(np.asarray(plane, np.float64) * 255.0).astype(np.uint8)


def _texcoords(T, w, h):
    u = (np.arange(w, dtype=T) + T(0.5)) / T(w)
    v = (np.arange(h, dtype=T) + T(0.5)) / T(h)
    return np.broadcast_to(u[None, :], (h, w)).astype(T), np.broadcast_to(v[:, None], (h, w)).astype(T)


def _to_int(x):
    """float -> int as v_cvt_i32_f32 does it: NaN -> 0, saturating at the ends of int32 (held in int64)"""
    nan = np.isnan(x)
    c = np.where(nan, 0.0, np.clip(np.where(nan, 0.0, x), -2147483648.0, 2147483647.0))
    return c.astype(np.int64)


def _sample(T, plane, u, v):
    """bilinear, clamp-to-edge: bilinear_taps + lerp2 of sailor_amd/csrc/sampling.h in the number type T"""
    h, w = plane.shape
    one, half = T(1.0), T(0.5)
    x = u * T(w) - half
    y = v * T(h) - half
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    x0 = np.clip(_to_int(fx), -1, w - 1)
    y0 = np.clip(_to_int(fy), -1, h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
    p = plane.astype(T)
    top = p[y0, x0] * (one - ax) + p[y0, x1] * ax
    bot = p[y1, x0] * (one - ax) + p[y1, x1] * ax
    return top * (one - ay) + bot * ay


def _store(T, v):
    c = np.where(np.isnan(v), T(0.0), np.where(v < 0, T(0.0), np.where(v > 1, T(1.0), v))).astype(T)
    return (np.rint(c * T(255.0)) / T(255.0)).astype(f32)


def _saturate(T, x):
    return np.where(x < 0, T(0.0), np.where(x > 1, T(1.0), x)).astype(T)


def _clip_to_view(T, M, u, v, d):
    """Math.glsl:143-154 with clip = (u, v, depth, 1); M[r][c] = element (row r, column c) of frame.invProjection"""
    row = lambda r: ((M[r][0] * u + M[r][1] * v) + M[r][2] * d) + M[r][3] * T(1.0)
    x, y, z, w = row(0), row(1), row(2), row(3)
    return x / w, y / w, -(z / w)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize3(v):
    l = np.sqrt(_dot3(v, v))
    return v[0] / l, v[1] / l, v[2] / l


def _hbao(T, literal_sin, frame, depth, noise, params, w, h):
    lit = lambda x: T(f32(x))
    one = T(1.0)
    depth = np.asarray(depth, f32)
    noise = np.asarray(noise, f32)
    dh, dw = depth.shape
    nh, nw = noise.shape[:2]
    P_ = {k: lit(params[k]) for k in SHIPPED}
    inv = np.array(list(frame.invProjection), f32)  # column-major
    M = [[T(inv[c * 4 + r]) for c in range(4)] for r in range(4)]
    z_near, viewport_h = T(f32(frame.cameraZNearZFar[0])), T(f32(frame.viewportSize[1]))
    size_x, size_y = T(dw), T(dh)
    inv_x, inv_y = one / size_x, one / size_y
    snap = lambda x, size, inv_size: np.rint(x * size) * inv_size  # :119-122

    with np.errstate(all="ignore"):
        u, v = _texcoords(T, w, h)
        d = _sample(T, depth, u, v)
        P = list(_clip_to_view(T, M, u, v, d))  # :187
        sky = P[2] > lit(49000.0)               # :190

        # :94-117, then :199
        uL, uR, vD, vU = u + T(-1.0) * inv_x, u + one * inv_x, v + T(-1.0) * inv_y, v + one * inv_y
        dL, dR, dD, dU = _sample(T, depth, uL, v), _sample(T, depth, uR, v), _sample(T, depth, u, vD), _sample(T, depth, u, vU)

        def smaller(left, mid, right):
            a, b = mid - left, right - mid
            return np.where(np.abs(a) < np.abs(b), a, b).astype(T)

        ddx, ddy = smaller(dL, d, dR), smaller(dD, d, dU)
        r = _clip_to_view(T, M, uR, v, d + ddx)
        t = _clip_to_view(T, M, u, vU, d + ddy)
        right = [r[k] - P[k] for k in range(3)]
        up = [t[k] - P[k] for k in range(3)]
        c = (up[1] * right[2] - right[1] * up[2], up[2] * right[0] - right[2] * up[0], up[0] * right[1] - right[0] * up[1])
        N = _normalize3(_normalize3(c))

        s = one + (lit(0.1) * P[2]) / z_near  # :201
        P = [P[k] + (N[k] * lit(0.00001)) * s for k in range(3)]

        kx = _to_int(np.floor((u * P_["noiseScale"]) * T(nw)))  # :203, nearest / repeat
        ky = _to_int(np.floor((v * P_["noiseScale"]) * T(nh)))
        nz = noise[np.mod(ky, nh), np.mod(kx, nw)].astype(T)
        off_x, off_y = (nz[..., 0] * T(2.0) - one) / T(4.0), (nz[..., 1] * T(2.0) - one) / T(4.0)
        jitter = nz[..., 1]

        sample_radius = P_["occlusionRadius"]  # :206-214: maxAORadius is NaN, min() returns its first argument
        ratio = size_y / viewport_h            # :222
        ssr = ((lit(50.0) * sample_radius) * ratio) / P[2]
        small = ssr < one                      # :225

        rad_x, rad_y = ssr * inv_x, ssr * inv_y
        R2 = P_["occlusionRadius"] * P_["occlusionRadius"]
        inv_R2, inv_att = one / R2, one / P_["occlusionAttenuation"]
        bias3 = P_["occlusionBias"] * T(3.0)
        inv9 = one / T(9.0)

        factor = np.zeros((h, w), T)
        for dx0, dy0 in DIRECTIONS:  # :234-245
            dir_x, dir_y = lit(dx0) + off_x, lit(dy0) + off_y
            dl = np.sqrt(dir_x * dir_x + dir_y * dir_y)
            dir_x, dir_y = dir_x / dl, dir_y / dl
            texel_x, texel_y = dir_x * inv_x, dir_y * inv_y  # :158
            dir_x, dir_y = dir_x * rad_x, dir_y * rad_y      # :159
            step_x, step_y = snap(dir_x * inv9, size_x, inv_x), snap(dir_y * inv9, size_y, inv_y)  # :162
            jit_x = texel_x * (one - jitter) + step_x * jitter
            jit_y = texel_y * (one - jitter) + step_y * jitter
            start_x, start_y = snap(u + jit_x, size_x, inv_x), snap(v + jit_y, size_y, inv_y)  # :164
            end_x, end_y = start_x + dir_x, start_y + dir_y
            occlusion = np.zeros((h, w), T)
            sin_h = np.full((h, w), P_["occlusionBias"], T)
            for step in range(8):  # :174-180
                tt = T(step) / T(8.0)
                su = snap(start_x * (one - tt) + end_x * tt, size_x, inv_x)
                sv = snap(start_y * (one - tt) + end_y * tt, size_y, inv_y)
                S = _clip_to_view(T, M, su, sv, _sample(T, depth, su, sv))
                hv = [S[k] - P[k] for k in range(3)]
                length = np.sqrt(_dot3(hv, hv))
                x = _dot3(N, [hv[k] / length for k in range(3)])
                sin_s = np.sin(T(np.pi) / T(2.0) - np.arccos(x)) if literal_sin else x  # :133
                hit = (length < R2) & (sin_s > sin_h + bias3)                            # :135
                falloff_z = one - _saturate(T, np.abs(hv[2]) * lit(0.007))
                distance_factor = one - (length * inv_R2) * inv_att
                occ = ((sin_s - sin_h) * distance_factor) * falloff_z
                occlusion = occlusion + np.where(hit, occ, T(0.0))
                sin_h = np.where(hit, sin_s, sin_h).astype(T)
            factor = factor + occlusion
        out = one - _saturate(T, (P_["occlusionPower"] / T(8.0)) * factor)  # :247
        out = np.where(sky | small, one, out)
        return _store(T, out)


def _blur_pass(T, exp2, ao, depth, params, w, h, vertical):
    lit = lambda x: T(f32(x))
    one = T(1.0)
    ao, depth = np.asarray(ao, f32), np.asarray(depth, f32)
    dh, dw = depth.shape
    sharpness, distance_scale, radius = lit(params["sharpness"]), lit(params["distanceScale"]), lit(params["radius"])
    pix_x, pix_y = (T(0.0), one / T(dh)) if vertical else (one / T(dw), T(0.0))  # HBAO_Blur.shader:84-90
    with np.errstate(all="ignore"):
        u, v = _texcoords(T, w, h)
        center_d = _sample(T, depth, u, v)
        total_c, total_w = _sample(T, ao, u, v), np.ones((h, w), T)
        sigma = radius * sharpness
        falloff = one / ((T(2.0) * sigma) * sigma)
        for sign in (1, -1):  # :98-108
            r = one
            while r <= radius:
                su, sv = (u + pix_x * r, v + pix_y * r) if sign > 0 else (u - pix_x * r, v - pix_y * r)
                c, d = _sample(T, ao, su, sv), _sample(T, depth, su, sv)
                diff = (d - center_d) * distance_scale
                wgt = exp2(((-r * r) * falloff) - diff * diff)
                total_w = total_w + wgt
                total_c = total_c + c * wgt
                r = r + one
        return _store(T, total_c / total_w)


class Ref32:
    dtype = f32
    blit = staticmethod(blit)

    @staticmethod
    def hbao(frame, depth, noise, params, w, h):
        return _hbao(f32, False, frame, depth, noise, params, w, h)

    @staticmethod
    def blur_pass(ao, depth, params, w, h, vertical):
        return _blur_pass(f32, canonical_exp2f, ao, depth, params, w, h, vertical)

    @classmethod
    def chain(cls, frame, depth, noise, params, blur_params, half_extent, ao_extent, temp_extent, out_extent):
        return _chain(cls, frame, depth, noise, params, blur_params, half_extent, ao_extent, temp_extent, out_extent)


class Ref64:
    dtype = np.float64
    blit = staticmethod(blit)

    @staticmethod
    def hbao(frame, depth, noise, params, w, h):
        return _hbao(np.float64, True, frame, depth, noise, params, w, h)

    @staticmethod
    def blur_pass(ao, depth, params, w, h, vertical):
        return _blur_pass(np.float64, np.exp2, ao, depth, params, w, h, vertical)

    @classmethod
    def chain(cls, frame, depth, noise, params, blur_params, half_extent, ao_extent, temp_extent, out_extent):
        return _chain(cls, frame, depth, noise, params, blur_params, half_extent, ao_extent, temp_extent, out_extent)


def _chain(R, frame, depth, noise, params, blur_params, half_extent, ao_extent, temp_extent, out_extent):
    """(HalfDepth, AO, TemporaryR8, g_AO); extents are (width, height)"""
    half = R.blit(depth, *half_extent)
    ao = R.hbao(frame, half, noise, params, *ao_extent)
    temp = R.blur_pass(ao, depth, blur_params, *temp_extent, True)
    out = R.blur_pass(temp, depth, blur_params, *out_extent, False)
    return half, ao, temp, out


def shipped_extents(width, height):
    """DefaultRenderer.renderer:46-72: HalfDepth and AO are ViewportWidth / 2 squared, TemporaryR8 and g_AO ViewportWidth squared"""
    return (width // 2, width // 2), (width // 2, width // 2), (width, width), (width, width)
