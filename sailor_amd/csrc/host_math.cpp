// Host-side math of the path (pure CPU): the glm-based camera / frustum / CSM set-up the reference does on the
// main and render threads before any GPU work is recorded.  glm itself is an un-vendored submodule of the reference
// (External/glm, .gitmodules:4-6); the few routines the path needs are written here against glm's published
// evaluation order so that frame constants are reproducible bit for bit.
//
//   PerspectiveRH (reversed Z)            Math/Math.cpp:18-21
//   glm::inverse                          ECS/CameraECS.cpp:20,33 ; ECS/LightingECS.cpp:227
//   Transform::Matrix                     Math/Transform.cpp:39-42
//   FillFrameData                         FrameGraph/RHIFrameGraph.cpp:60-67
//   Frustum::ExtractFrustumPlanes         Math/Bounds.cpp:142-193
//   CalculateOrthoMatrixByView            Math/Bounds.cpp:78-109
//   CalculateLightProjectionForCascades   FrameGraph/ShadowPrepassNode.cpp:387-404 (+ ECS/LightingECS.cpp:292)
//   LightShaderData packing               ECS/LightingECS.cpp:163-172
#define SAILOR_HIP_BUILD 1
#include "../../include/sailor_hip.h"
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <new>
#include <algorithm>
#include <limits>

namespace {

struct V3 {
    float x, y, z;
};
struct V4 {
    float x, y, z, w;
    float& operator[](int i) { return (&x)[i]; }
    float operator[](int i) const { return (&x)[i]; }
};
inline V4 operator*(const V4& a, float s) { return { a.x * s, a.y * s, a.z * s, a.w * s }; }
inline V4 operator+(const V4& a, const V4& b) { return { a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w }; }
inline V3 operator*(const V3& a, float s) { return { a.x * s, a.y * s, a.z * s }; }
inline V3 operator*(float s, const V3& a) { return { s * a.x, s * a.y, s * a.z }; }
inline V3 operator+(const V3& a, const V3& b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline V3 operator-(const V3& a, const V3& b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline V3 operator-(const V3& a) { return { -a.x, -a.y, -a.z }; }

struct M4 {
    V4 c[4]; // columns, as glm::mat4
    V4& operator[](int i) { return c[i]; }
    const V4& operator[](int i) const { return c[i]; }
};

inline M4 load(const float* p) { M4 m; std::memcpy(&m, p, 64); return m; }
inline void store(const M4& m, float* p) { std::memcpy(p, &m, 64); }
inline M4 identity() { return { { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 }, { 0, 0, 0, 1 } } }; }

// glm: operator*(mat4, mat4) -- column c = A0*B[c].x + A1*B[c].y + A2*B[c].z + A3*B[c].w, summed left to right
inline M4 mul(const M4& a, const M4& b)
{
    M4 r;
    for (int c = 0; c < 4; c++) r[c] = ((a[0] * b[c].x + a[1] * b[c].y) + a[2] * b[c].z) + a[3] * b[c].w;
    return r;
}
// glm: operator*(mat4, vec4) -- (m0*v.x + m1*v.y) + (m2*v.z + m3*v.w)
inline V4 mul(const M4& m, const V4& v) { return (m[0] * v.x + m[1] * v.y) + (m[2] * v.z + m[3] * v.w); }

inline float dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(const V3& x, const V3& y) { return { x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y }; }
inline V3 normalize(const V3& v) { return v * (1.0f / std::sqrt(dot(v, v))); } // v * inversesqrt(dot(v, v))

// glm compute_inverse<4, 4>
M4 inverse(const M4& m)
{
    const float c00 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c02 = m[1][2] * m[3][3] - m[3][2] * m[1][3], c03 = m[1][2] * m[2][3] - m[2][2] * m[1][3];
    const float c04 = m[2][1] * m[3][3] - m[3][1] * m[2][3], c06 = m[1][1] * m[3][3] - m[3][1] * m[1][3], c07 = m[1][1] * m[2][3] - m[2][1] * m[1][3];
    const float c08 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c10 = m[1][1] * m[3][2] - m[3][1] * m[1][2], c11 = m[1][1] * m[2][2] - m[2][1] * m[1][2];
    const float c12 = m[2][0] * m[3][3] - m[3][0] * m[2][3], c14 = m[1][0] * m[3][3] - m[3][0] * m[1][3], c15 = m[1][0] * m[2][3] - m[2][0] * m[1][3];
    const float c16 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c18 = m[1][0] * m[3][2] - m[3][0] * m[1][2], c19 = m[1][0] * m[2][2] - m[2][0] * m[1][2];
    const float c20 = m[2][0] * m[3][1] - m[3][0] * m[2][1], c22 = m[1][0] * m[3][1] - m[3][0] * m[1][1], c23 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
    const V4 f0 { c00, c00, c02, c03 }, f1 { c04, c04, c06, c07 }, f2 { c08, c08, c10, c11 };
    const V4 f3 { c12, c12, c14, c15 }, f4 { c16, c16, c18, c19 }, f5 { c20, c20, c22, c23 };
    const V4 v0 { m[1][0], m[0][0], m[0][0], m[0][0] }, v1 { m[1][1], m[0][1], m[0][1], m[0][1] };
    const V4 v2 { m[1][2], m[0][2], m[0][2], m[0][2] }, v3 { m[1][3], m[0][3], m[0][3], m[0][3] };
    auto had = [](const V4& a, const V4& b) { return V4 { a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w }; };
    auto sub = [](const V4& a, const V4& b) { return V4 { a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w }; };
    const V4 i0 = sub(had(v1, f0), had(v2, f1)) + had(v3, f2);
    const V4 i1 = sub(had(v0, f0), had(v2, f3)) + had(v3, f4);
    const V4 i2 = sub(had(v0, f1), had(v1, f3)) + had(v3, f5);
    const V4 i3 = sub(had(v0, f2), had(v1, f4)) + had(v2, f5);
    const V4 sa { +1, -1, +1, -1 }, sb { -1, +1, -1, +1 };
    M4 inv { { had(i0, sa), had(i1, sb), had(i2, sa), had(i3, sb) } };
    const V4 row0 { inv[0][0], inv[1][0], inv[2][0], inv[3][0] };
    const V4 d0 = had(m[0], row0);
    const float d1 = (d0.x + d0.y) + (d0.z + d0.w);
    const float ood = 1.0f / d1;
    for (int c = 0; c < 4; c++) inv[c] = inv[c] * ood;
    return inv;
}

// glm::perspectiveRH_ZO
M4 perspective_rh_zo(float fovy, float aspect, float zNear, float zFar)
{
    const float t = std::tan(fovy / 2.0f);
    M4 r {};
    r[0][0] = 1.0f / (aspect * t);
    r[1][1] = 1.0f / t;
    r[2][2] = zFar / (zNear - zFar);
    r[2][3] = -1.0f;
    r[3][2] = -(zFar * zNear) / (zFar - zNear);
    return r;
}

// glm::orthoRH_NO
M4 ortho_rh_no(float left, float right, float bottom, float top, float zNear, float zFar)
{
    M4 r = identity();
    r[0][0] = 2.0f / (right - left);
    r[1][1] = 2.0f / (top - bottom);
    r[2][2] = -2.0f / (zFar - zNear);
    r[3][0] = -(right + left) / (right - left);
    r[3][1] = -(top + bottom) / (top - bottom);
    r[3][2] = -(zFar + zNear) / (zFar - zNear);
    return r;
}

// glm::translate(mat4(1), v): Result[3] = m[0]*v[0] + m[1]*v[1] + m[2]*v[2] + m[3]
M4 translation(const float* v)
{
    const M4 I = identity();
    M4 T = I;
    T[3] = ((I[0] * v[0] + I[1] * v[1]) + I[2] * v[2]) + I[3];
    return T;
}
// glm::mat4_cast(quat)
M4 mat4_cast(float x, float y, float z, float w)
{
    const float qxx = x * x, qyy = y * y, qzz = z * z, qxz = x * z, qxy = x * y, qyz = y * z, qwx = w * x, qwy = w * y, qwz = w * z;
    M4 R = identity();
    R[0][0] = 1.0f - 2.0f * (qyy + qzz); R[0][1] = 2.0f * (qxy + qwz); R[0][2] = 2.0f * (qxz - qwy);
    R[1][0] = 2.0f * (qxy - qwz); R[1][1] = 1.0f - 2.0f * (qxx + qzz); R[1][2] = 2.0f * (qyz + qwx);
    R[2][0] = 2.0f * (qxz + qwy); R[2][1] = 2.0f * (qyz - qwx); R[2][2] = 1.0f - 2.0f * (qxx + qyy);
    return R;
}

M4 transform_matrix(const SailorTransform& t)
{
    const M4 I = identity();
    const M4 T = translation(t.position);
    const M4 R = mat4_cast(t.rotation[0], t.rotation[1], t.rotation[2], t.rotation[3]); // quat memory order x,y,z,w
    // glm::scale(m, v): Result[i] = m[i] * v[i]; Result[3] = m[3]
    M4 S;
    S[0] = I[0] * t.scale[0]; S[1] = I[1] * t.scale[1]; S[2] = I[2] * t.scale[2]; S[3] = I[3];
    return mul(mul(T, R), S);
}

struct Plane {
    V4 abcd;
    Plane() : abcd { 0, 0, 0, 0 } {}
    Plane(const V3& n, const V3& p) : abcd { n.x, n.y, n.z, -dot(p, n) } {} // Bounds.h:80-87
    void normalize()
    { // Bounds.cpp:9-13
        const float mag = std::sqrt(dot(V3 { abcd.x, abcd.y, abcd.z }, V3 { abcd.x, abcd.y, abcd.z }));
        abcd.x /= mag; abcd.y /= mag; abcd.z /= mag; abcd.w /= mag;
    }
};

struct Frustum {
    Plane planes[6]; // L R T B N F
    V3 corners[8];
    // Bounds.cpp:142-193
    void extract(const M4& world, float aspect, float fovY, float zNear, float zFar)
    {
        const float radians = fovY * 0.01745329251994329576923690768489f;
        const float halfVSide = zFar * std::tan(radians * .5f);
        const float halfHSide = halfVSide * aspect;
        const V3 right { world[0].x, world[0].y, world[0].z };
        const V3 up { world[1].x, world[1].y, world[1].z };
        const V3 forward = -V3 { world[2].x, world[2].y, world[2].z };
        const V3 pos { world[3].x, world[3].y, world[3].z };
        const V3 frontMultFar = zFar * forward;
        planes[4] = Plane(forward, pos + forward * zNear);
        planes[5] = Plane(-forward, pos + forward * zFar);
        planes[0] = Plane(normalize(cross(frontMultFar - right * halfHSide, up)), pos);
        planes[1] = Plane(normalize(cross(up, frontMultFar + right * halfHSide)), pos);
        const V3 bottomNormal = normalize(cross(right, frontMultFar - up * halfVSide));
        const V3 topNormal = normalize(cross(frontMultFar + up * halfVSide, right));
        planes[2] = Plane(topNormal, pos);
        planes[3] = Plane(bottomNormal, pos);
        for (auto& p : planes) p.normalize();

        const V3 farEnd { 0, 0, -zFar }, eh { halfHSide, 0, 0 }, ev { 0, halfVSide, 0 };
        auto xf = [&](const V3& v) { const V4 r = mul(world, V4 { v.x, v.y, v.z, 1.0f }); return V3 { r.x, r.y, r.z }; };
        corners[0] = xf(farEnd + eh + ev);
        corners[1] = xf(farEnd - eh + ev);
        corners[2] = xf(farEnd - eh - ev);
        corners[3] = xf(farEnd + eh - ev);
        const float halfVSideNear = zNear * std::tan(radians * .5f);
        const float halfHSideNear = halfVSideNear * aspect;
        const V3 start { 0, 0, -zNear }, sx { halfHSideNear, 0, 0 }, sy { 0, halfVSideNear, 0 };
        corners[4] = xf(start + sx + sy);
        corners[5] = xf(start - sx + sy);
        corners[6] = xf(start - sx - sy);
        corners[7] = xf(start + sx - sy);
    }
    // Bounds.cpp:20-67 ExtractFrustumPlanes(projectionViewMatrix) with :110-140 CalculateCorners(matrix, bReverseZ = true)
    void extract(const M4& projectionView)
    {
        const M4 inv = inverse(projectionView);
        const float sgn[4][2] = { { 1.0f, 1.0f }, { -1.0f, 1.0f }, { -1.0f, -1.0f }, { 1.0f, -1.0f } };
        for (int k = 0; k < 8; k++) {
            const float reverseZ = -1.0f;
            const V4 pt = mul(inv, V4 { sgn[k & 3][0], sgn[k & 3][1], k < 4 ? reverseZ * 1.0f : reverseZ * -1.0f, 1.0f });
            corners[k] = V3 { pt.x / pt.w, pt.y / pt.w, pt.z / pt.w };
        }
        const V3 right = normalize(corners[0] - corners[1]), up = normalize(corners[0] - corners[3]), forward = normalize(corners[0] - corners[4]);
        const V3 centerFar = 0.5f * (corners[0] + corners[2]), centerNear = 0.5f * (corners[4] + corners[6]);
        const V3 centerBottom = 0.5f * (corners[2] + corners[7]), centerTop = 0.5f * (corners[0] + corners[5]);
        const V3 centerLeft = 0.5f * (corners[1] + corners[6]), centerRight = 0.5f * (corners[0] + corners[7]);
        planes[4] = Plane(forward, centerNear);
        planes[5] = Plane(-forward, centerFar);
        planes[0] = Plane(normalize(cross(forward, up)), centerLeft);
        planes[1] = Plane(normalize(cross(up, forward)), centerRight);
        planes[2] = Plane(normalize(cross(forward, right)), centerTop);
        planes[3] = Plane(normalize(cross(right, forward)), centerBottom);
        for (auto& p : planes) p.normalize();
    }
    // Bounds.cpp:78-109
    M4 ortho_by_view(const M4& view, float zMult) const
    {
        float minX = std::numeric_limits<float>::max(), maxX = std::numeric_limits<float>::lowest();
        float minY = minX, maxY = maxX, minZ = minX, maxZ = maxX;
        for (const V3& v : corners) {
            const V4 t = mul(view, V4 { v.x, v.y, v.z, 1 });
            minX = std::min(minX, t.x); maxX = std::max(maxX, t.x);
            minY = std::min(minY, t.y); maxY = std::max(maxY, t.y);
            minZ = std::min(minZ, t.z); maxZ = std::max(maxZ, t.z);
        }
        minZ = minZ < 0 ? minZ * zMult : minZ / zMult;
        maxZ = maxZ < 0 ? maxZ / zMult : maxZ * zMult;
        const float zFar = -minZ, zNear = -maxZ;
        return ortho_rh_no(minX, maxX, minY, maxY, zFar, zNear); // reversed Z for shadows
    }
};

constexpr float kShadowCascadeLevels[SAILOR_NUM_CSM_CASCADES] = { 1.0f / 20.0f, 1.0f / 10.0f, 1.0f / 3.0f, 1.0f / 2.0f }; // ECS/LightingECS.h:66

} // namespace

extern "C" {

int sailor_host_perspective_rh(float fovRadians, float aspect, float zNear, float zFar, float* outMat4)
{
    if (!outMat4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    store(perspective_rh_zo(fovRadians, aspect, zFar, zNear), outMat4); // Math.cpp:20: near/far swapped
    return SAILOR_HIP_OK;
}

int sailor_host_mat4_inverse(const float* m, float* outMat4)
{
    if (!m || !outMat4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    store(inverse(load(m)), outMat4);
    return SAILOR_HIP_OK;
}

int sailor_host_mat4_mul(const float* a, const float* b, float* outMat4)
{
    if (!a || !b || !outMat4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    store(mul(load(a), load(b)), outMat4);
    return SAILOR_HIP_OK;
}

int sailor_host_transform_matrix(const SailorTransform* t, float* outMat4)
{
    if (!t || !outMat4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    store(transform_matrix(*t), outMat4);
    return SAILOR_HIP_OK;
}

int sailor_host_fill_frame_data(const float* cameraWorld, float fovDegrees, float aspect, float zNear, float zFar,
                                int32_t viewportWidth, int32_t viewportHeight, float currentTime, float deltaTime, SailorUboFrameData* outFrame)
{
    if (!cameraWorld || !outFrame || viewportWidth <= 0 || viewportHeight <= 0) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const M4 world = load(cameraWorld);
    const M4 view = mul(identity(), inverse(world)); // CameraECS.cpp:19-20: origin * inverse(world)
    const M4 proj = perspective_rh_zo(fovDegrees * 0.01745329251994329576923690768489f, aspect, zFar, zNear); // CameraComponent: radians(fov)
    const M4 invProj = inverse(proj);                                                                          // CameraECS.cpp:31-34
    store(view, outFrame->view);
    store(proj, outFrame->projection);
    store(invProj, outFrame->invProjection);
    outFrame->cameraPosition[0] = world[3].x; outFrame->cameraPosition[1] = world[3].y;
    outFrame->cameraPosition[2] = world[3].z; outFrame->cameraPosition[3] = world[3].w;
    outFrame->viewportSize[0] = viewportWidth; outFrame->viewportSize[1] = viewportHeight;
    outFrame->cameraZNearZFar[0] = zNear; outFrame->cameraZNearZFar[1] = zFar;
    outFrame->currentTime = currentTime; outFrame->deltaTime = deltaTime;
    return SAILOR_HIP_OK;
}

int sailor_host_extract_frustum_planes(const float* worldMatrix, float aspect, float fovYDegrees, float zNear, float zFar, float* outPlanes24, float* outCorners24)
{
    if (!worldMatrix || !outPlanes24) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    Frustum f;
    f.extract(load(worldMatrix), aspect, fovYDegrees, zNear, zFar);
    for (int i = 0; i < 6; i++) std::memcpy(outPlanes24 + 4 * i, &f.planes[i].abcd, 16);
    if (outCorners24) std::memcpy(outCorners24, f.corners, sizeof f.corners);
    return SAILOR_HIP_OK;
}

int sailor_host_extract_frustum_planes_matrix(const float* projectionViewMatrix, float* outPlanes24, float* outCorners24)
{
    if (!projectionViewMatrix || !outPlanes24) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    Frustum f;
    f.extract(load(projectionViewMatrix));
    for (int i = 0; i < 6; i++) std::memcpy(outPlanes24 + 4 * i, &f.planes[i].abcd, 16);
    if (outCorners24) std::memcpy(outCorners24, f.corners, sizeof f.corners);
    return SAILOR_HIP_OK;
}

int sailor_host_csm_matrices(const float* lightView, const float* cameraWorld, float aspect, float fovYDegrees, float cameraNear, float cameraFar, float* outMatrices64)
{
    if (!lightView || !cameraWorld || !outMatrices64) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const M4 lv = load(lightView), cw = load(cameraWorld);
    for (int k = 0; k < SAILOR_NUM_CSM_CASCADES; k++) {
        // ShadowPrepassNode.cpp:392-400: cascade 0 spans [near, far*L0], cascade k spans [far*L(k-1), far*Lk]; zMult 10
        const float n = k == 0 ? cameraNear : cameraFar * kShadowCascadeLevels[k - 1];
        const float f = cameraFar * kShadowCascadeLevels[k];
        Frustum fr;
        fr.extract(cw, aspect, fovYDegrees, n, f);
        const M4 ortho = fr.ortho_by_view(lv, 10.0f);
        store(mul(ortho, lv), outMatrices64 + 16 * k); // LightingECS.cpp:292
    }
    return SAILOR_HIP_OK;
}

int sailor_host_pack_light(uint32_t type, uint32_t shadowType, const float* worldPosition, const float* direction, const float* intensity,
                           const float* attenuation, const float* cutOffDegrees, const float* bounds, SailorLightShaderData* outLight)
{
    if (!worldPosition || !direction || !intensity || !attenuation || !cutOffDegrees || !bounds || !outLight) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    std::memset(outLight, 0, sizeof *outLight);
    outLight->type = type;
    outLight->shadowType = shadowType;
    for (int i = 0; i < 3; i++) {
        outLight->worldPosition[i] = worldPosition[i];
        outLight->direction[i] = direction[i];
        outLight->intensity[i] = intensity[i];
        outLight->attenuation[i] = attenuation[i];
        outLight->bounds[i] = bounds[i];
    }
    // LightingECS.cpp:171: vec2(cos(radians(cutOff.x)), cos(radians(cutOff.y)))
    outLight->cutOff[0] = std::cos(cutOffDegrees[0] * 0.01745329251994329576923690768489f);
    outLight->cutOff[1] = std::cos(cutOffDegrees[1] * 0.01745329251994329576923690768489f);
    return SAILOR_HIP_OK;
}

// ---- FrameGraph/EyeAdaptationNode.cpp:154-170: the push constants of the histogram and the average Dispatch ----
int sailor_host_eye_adaptation_constants(int32_t width, int32_t height, float deltaTime, SailorEyeAdaptationConstants* outConstants)
{
    if (width <= 0 || height <= 0 || !outConstants) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const float minLogLuminance = -8.0f, maxLogLuminance = 4.0f, eyeReaction = 3.6f; // :154-156
    const float logLuminanceRange = maxLogLuminance - minLogLuminance;               // :158
    outConstants->minLog2Luminance = minLogLuminance;
    outConstants->invLog2LuminanceRange = 1.0f / logLuminanceRange;                  // :160
    outConstants->log2LuminanceRange = logLuminanceRange;
    outConstants->numPixels = (float)width * height;                                 // :168
    outConstants->timeCoeff = std::clamp(1.0f - std::exp2(-deltaTime * eyeReaction), 0.0f, 1.0f); // :162
    return SAILOR_HIP_OK;
}

// ---- FrameGraph/BloomNode.cpp:89-93: the downscale's u_threshold ----
int sailor_host_bloom_push_constants(float threshold, float knee, float* outThreshold4)
{
    if (!outThreshold4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    outThreshold4[0] = threshold;
    outThreshold4[1] = threshold - knee;
    outThreshold4[2] = 2.0f * knee;
    outThreshold4[3] = 0.25f * knee;
    return SAILOR_HIP_OK;
}

// ---- Math/Bounds.cpp:211-243: the scalar sphere tests; their only caller is LightingECS::GetLightsInFrustum (ContainsSphere, :237) ----
int sailor_host_overlaps_sphere(const float* planes24, const float* sphere4)
{
    if (!planes24 || !sphere4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    int res = 1;
    for (int p = 0; p < 6; p++)
        if (planes24[4 * p + 0] * sphere4[0] + planes24[4 * p + 1] * sphere4[1] + planes24[4 * p + 2] * sphere4[2] + planes24[4 * p + 3] < -sphere4[3]) res = 0;
    return res;
}

int sailor_host_contains_sphere(const float* planes24, const float* sphere4)
{
    if (!planes24 || !sphere4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    int res = 1;
    for (int p = 0; p < 6; p++)
        if (planes24[4 * p + 0] * sphere4[0] + planes24[4 * p + 1] * sphere4[1] + planes24[4 * p + 2] * sphere4[2] + planes24[4 * p + 3] < sphere4[3]) res = 0;
    return res;
}

// ---- ECS/LightingECS.cpp:209-260 GetLightsInFrustum: the shadow-casting lights of a view.  Directional lights in component order; point
// and spot lights whose bounding sphere (radius = the largest bound) lies INSIDE the frustum, each list sorted by distance to the camera
// through the reference's own insertion: position = std::lower_bound(list, proxy) under operator< on the distance, i.e. a light goes
// in FRONT of the lights already there at the same distance.
int sailor_host_lights_in_frustum(const float* planes24, const float* cameraPosition3, uint32_t numLights, const uint32_t* types, const uint32_t* shadowTypes,
                                  const uint8_t* active, const float* positions3, const float* bounds3,
                                  uint32_t* outDirectional, uint32_t* outNumDirectional,
                                  uint32_t* outPoint, float* outPointDistance, uint32_t* outNumPoint,
                                  uint32_t* outSpot, float* outSpotDistance, uint32_t* outNumSpot)
{
    if (!planes24 || !cameraPosition3 || (numLights && (!types || !shadowTypes || !positions3 || !bounds3)) || !outDirectional || !outNumDirectional || !outPoint ||
        !outPointDistance || !outNumPoint || !outSpot || !outSpotDistance || !outNumSpot)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    uint32_t nd = 0, np = 0, ns = 0;
    auto insert = [](uint32_t* idx, float* dist, uint32_t& n, uint32_t index, float d) {
        uint32_t lo = 0, hi = n; // lower_bound: first element that is not < d
        while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (dist[mid] < d) lo = mid + 1; else hi = mid; }
        for (uint32_t k = n; k > lo; k--) { idx[k] = idx[k - 1]; dist[k] = dist[k - 1]; }
        idx[lo] = index; dist[lo] = d; n++;
    };
    for (uint32_t i = 0; i < numLights; i++) {
        if (shadowTypes[i] == 0u /* EShadowType::None */ || (active && !active[i])) continue; // :222
        if (types[i] == 0u /* Directional */) { outDirectional[nd++] = i; continue; }           // :255
        const float* b = bounds3 + 3 * (size_t)i;
        const float* p = positions3 + 3 * (size_t)i;
        const float sphere[4] = { p[0], p[1], p[2], std::max(std::max(b[0], b[1]), b[2]) };     // :235
        if (!sailor_host_contains_sphere(planes24, sphere)) continue;                            // :237
        const float dx = p[0] - cameraPosition3[0], dy = p[1] - cameraPosition3[1], dz = p[2] - cameraPosition3[2];
        const float d = std::sqrt((dx * dx + dy * dy) + dz * dz);                                // :240 glm::length
        if (types[i] == 2u /* Spot */) insert(outSpot, outSpotDistance, ns, i, d);
        else insert(outPoint, outPointDistance, np, i, d);
    }
    *outNumDirectional = nd; *outNumPoint = np; *outNumSpot = ns;
    return SAILOR_HIP_OK;
}

} // extern "C"

// ---- FrameGraph/SkyNode.cpp:31-91, :836-875 and Core/Utils.cpp:454-464: the star mesh of the Sky node from the Bright Star Catalogue ----------------
// The reference indexes out of range on real data: the shipped catalogue holds the spectral bytes ' ' and 'p' (s_starTemperatureRanges[spectralType -
// 'A'] has 25 entries for 'A' .. 'Y') and the sub-type bytes m p e N I C + / and space ('9' - subType wraps), and clamp(index, 0, 390) addresses
// s_rgbTemperatures[390].  Decisions:
//   * the integer arithmetic wraps in uint32 as written: subIndex = '9' - subType, subIndex * rangeStep, temperature / 100 - 10 reinterpreted as int32;
//   * a float -> integer conversion saturates (NaN -> 0): uint32_t(x) into [0, 2^32 - 1];
//   * a spectral byte outside 'A' .. 'Y' takes the range {0, 0};
//   * the table has 391 entries, so that both clamps (:52: min(index, 390u); :866: clamp(index, 0, 390)) address it;
//   * no byte pattern indexes outside a table or reads past `bytes`: a catalogue shorter than its header, or than the entries its header counts, is refused.
namespace {
constexpr uint32_t kMaxRgbTemperatures = (40000 / 100) - (1000 / 100); // SkyNode.h:163
constexpr size_t kStarHeaderBytes = 28, kStarEntryBytes = 32;          // SkyNode.h:20-44: seven int32; float, double, double, char[2], int16, float, float packed

uint32_t saturating_u32(float x)
{
    if (!(x > 0.0f)) return 0u; // NaN, zero and the negatives
    if (x >= 4294967296.0f) return 4294967295u;
    return (uint32_t)x;
}

// MorganKeenanToTemperature (:836-861)
uint32_t morgan_keenan_temperature(uint8_t spectralType, uint8_t subType)
{
    static const float ranges[25][2] = {
        { 7300, 10000 }, { 10000, 30000 }, { 2400, 3200 }, { 100000, 1000000 }, { 0, 0 }, { 6000, 7300 }, { 5300, 6000 }, { 0, 0 }, { 0, 0 },
        { 0, 0 }, { 3800, 5300 }, { 1300, 2100 }, { 2500, 3800 }, { 0, 0 }, { 30000, 40000 }, { 0, 0 }, { 0, 0 }, { 0, 0 }, { 2400, 3500 }, { 600, 1300 },
        { 0, 0 }, { 0, 0 }, { 25000, 40000 }, { 0, 0 }, { 0, 600 } };
    static const float none[2] = { 0, 0 };
    const float* range = spectralType >= 'A' && spectralType <= 'Y' ? ranges[spectralType - 'A'] : none;
    const uint32_t rangeStep = saturating_u32((range[1] - range[0]) / 9);
    const uint32_t subIndex = (uint32_t)'9' - (uint32_t)(int32_t)(int8_t)subType; // char is signed where the reference is built
    return saturating_u32(range[0] + (float)(subIndex * rangeStep));
}

// TemperatureToColor (:863-869): the row of the 391-entry table
uint32_t temperature_row(uint32_t temperature)
{
    const int32_t index = (int32_t)((temperature / 100u) - 10u);
    return (uint32_t)std::min(std::max(index, 0), (int32_t)kMaxRgbTemperatures);
}
} // namespace

extern "C" {

int sailor_host_sky_star_color_table(const float* rows, uint32_t rowCount, float* outTable)
{
    if ((rowCount && !rows) || !outTable) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    std::memset(outTable, 0, sizeof(float) * 3 * (kMaxRgbTemperatures + 1)); // s_rgbTemperatures is a static: zero-initialised
    for (uint32_t i = 0; i < rowCount; i++) {
        const float* line = rows + 11 * (size_t)i;
        const uint32_t index = std::min(saturating_u32((line[0] / 100.0f) - 10.0f), kMaxRgbTemperatures); // :51-52
        for (int c = 0; c < 3; c++) outTable[3 * index + c] = line[5 + c];                                 // :55-57
    }
    return SAILOR_HIP_OK;
}

int sailor_host_sky_star_mesh(const uint8_t* catalogue, size_t bytes, const float* table, float* outPositions, float* outColors, uint32_t capacity,
                              uint32_t* outCount)
{
    if (!catalogue || !table || !outCount || bytes < kStarHeaderBytes) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    int32_t starCount;
    std::memcpy(&starCount, catalogue + 8, 4);                                   // m_starCount
    const uint64_t count = (uint64_t)std::llabs((long long)starCount);           // :66 abs(header->m_starCount)
    if (count > (bytes - kStarHeaderBytes) / kStarEntryBytes) return SAILOR_HIP_ERR_INVALID_ARGUMENT; // a truncated catalogue
    *outCount = (uint32_t)count;
    if (count > capacity) return SAILOR_HIP_ERR_INVALID_ARGUMENT;                // (outCount says how much room the mesh needs)
    if (count && (!outPositions || !outColors)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < count; i++) {
        const uint8_t* e = catalogue + kStarHeaderBytes + kStarEntryBytes * i;
        double sra0, sdec0;
        int16_t mag;
        std::memcpy(&sra0, e + 4, 8); std::memcpy(&sdec0, e + 12, 8); std::memcpy(&mag, e + 22, 2);
        const float ra = (float)sra0, dec = (float)sdec0;                        // :76
        const float cosd = cosf(dec);                                            // Utils.cpp:454-464, radialDistance = 1
        float p[3] = { (1.0f * sinf(ra)) * cosd, (1.0f * cosf(ra)) * cosd, 1.0f * sinf(dec) };
        const float divisor = ((float)mag / 100.0f) + 0.4f;                      // :77; a negative divisor mirrors the star, as written
        for (int c = 0; c < 3; c++) outPositions[3 * i + c] = (p[c] / divisor) * 5000.0f; // :79-81
        const float* rgb = table + 3 * (size_t)temperature_row(morgan_keenan_temperature(e[20], e[21])); // :83
        const float color[4] = { rgb[0], rgb[1], rgb[2], 1.0f };
        for (int c = 0; c < 4; c++) outColors[4 * i + c] = powf(color[c], 1 / 2.2f); // :85-88
    }
    return SAILOR_HIP_OK;
}

int sailor_host_sky_stars_model(const float* cameraPosition3, float* outMat4)
{
    if (!cameraPosition3 || !outMat4) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    // SkyNode.cpp:208-209: glm::angleAxis(angle, axis) = (axis * sin(angle / 2), cos(angle / 2)); Math::vec3_Backward = (0, 0, 1), vec3_Right = (1, 0, 0)
    struct Q { float w, x, y, z; };
    auto angleAxis = [](float angle, float ax, float ay, float az) { const float s = sinf(angle * 0.5f); return Q { cosf(angle * 0.5f), ax * s, ay * s, az * s }; };
    auto qmul = [](const Q& p, const Q& q) { // glm: operator*(qua, qua)
        return Q { p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z, p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
                   p.w * q.y + p.y * q.w + p.z * q.x - p.x * q.z, p.w * q.z + p.z * q.w + p.x * q.y - p.y * q.x };
    };
    const Q rz = angleAxis(0.01118f, 0.0f, 0.0f, 1.0f);
    const Q q = qmul(qmul(rz, angleAxis(-0.00972f, 1.0f, 0.0f, 0.0f)), rz);
    // :211 toMat4(precession) and :698 translate(mat4(1), cameraPosition) * it
    store(mul(translation(cameraPosition3), mat4_cast(q.x, q.y, q.z, q.w)), outMat4);
    return SAILOR_HIP_OK;
}

} // extern "C"

// ---- ECS/LightingECS.cpp:14-38 CSMLightState + :299-366, the change tracking of LightingECS::PrepareCSMPasses -------------------------
namespace {
struct CsmLightState {
    bool hasView = false;
    SailorCsmView view {};
    std::vector<uint32_t> meshes;  // m_snapshot: (static mesh index, frame the mesh last changed)
    std::vector<uint64_t> frames;
};
static void quat_rotate(const float* q, const float* v, float* o) // glm: v + ((cross(q.xyz, v) * q.w) + cross(q.xyz, cross(q.xyz, v))) * 2 (Transform::GetForward)
{
    const float uv[3] = { q[1] * v[2] - v[1] * q[2], q[2] * v[0] - v[2] * q[0], q[0] * v[1] - v[0] * q[1] };
    const float uuv[3] = { q[1] * uv[2] - uv[1] * q[2], q[2] * uv[0] - uv[2] * q[0], q[0] * uv[1] - uv[0] * q[1] };
    for (int i = 0; i < 3; i++) o[i] = v[i] + ((uv[i] * q[3]) + uuv[i]) * 2.0f;
}
// the transform half of CSMLightState::Equals (:19-24)
static bool view_unchanged(bool hasA, const SailorCsmView& a, bool hasB, const SailorCsmView& b)
{
    if (!hasA || !hasB) return !hasA && !hasB;
    if (a.componentIndex != b.componentIndex) return false;
    float d2 = 0.0f;
    for (int i = 0; i < 4; i++) { const float d = a.cameraPosition[i] - b.cameraPosition[i]; d2 += d * d; }
    if (std::sqrt(d2) > 15.0f) return false;                         // CameraPosDelta
    const float fwd[3] = { 0.0f, 0.0f, -1.0f };
    float fa[3], fb[3];
    quat_rotate(a.cameraRotation, fwd, fa); quat_rotate(b.cameraRotation, fwd, fb);
    if ((fa[0] * fb[0] + fa[1] * fb[1]) + fa[2] * fb[2] < 0.9995f) return false; // CameraRotationDelta
    for (int i = 0; i < 4; i++)
        if (a.lightPosition[i] != b.lightPosition[i] || a.lightRotation[i] != b.lightRotation[i]) return false;
    return true;
}
} // namespace

struct SailorCsmSnapshots { std::vector<CsmLightState> states; }; // LightingECS::m_csmSnapshots

extern "C" {

SailorCsmSnapshots* sailor_host_csm_snapshots_create(void) { return new (std::nothrow) SailorCsmSnapshots(); }
SailorCsmSnapshots* sailor_host_csm_snapshots_clone(const SailorCsmSnapshots* s) { return s ? new (std::nothrow) SailorCsmSnapshots(*s) : nullptr; }
void sailor_host_csm_snapshots_destroy(SailorCsmSnapshots* s) { delete s; }
uint32_t sailor_host_csm_snapshots_count(const SailorCsmSnapshots* s) { return s ? (uint32_t)s->states.size() : 0u; }

int sailor_host_csm_snapshot_get(const SailorCsmSnapshots* s, uint32_t k, uint32_t capacity, uint32_t* outCount, uint32_t* outMeshes, uint64_t* outFrames,
                                 int32_t* outHasView, SailorCsmView* outView)
{
    if (!s || k >= s->states.size() || !outCount) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const CsmLightState& st = s->states[k];
    *outCount = (uint32_t)st.meshes.size();
    for (uint32_t i = 0; i < st.meshes.size() && i < capacity; i++) {
        if (outMeshes) outMeshes[i] = st.meshes[i];
        if (outFrames) outFrames[i] = st.frames[i];
    }
    if (outHasView) *outHasView = st.hasView ? 1 : 0;
    if (outView) *outView = st.view;
    return SAILOR_HIP_OK;
}

int sailor_host_csm_plan_passes(SailorCsmSnapshots* state, uint32_t firstSnapshot, uint32_t numCascades, uint32_t numEntities, const uint64_t* overlapMasks,
                                const uint32_t* shadowTypes, const uint64_t* lastChangedFrame, const SailorCsmView* view, uint32_t* outRender, uint64_t* outMasks)
{
    if (!state || !overlapMasks || !shadowTypes || (numEntities && !lastChangedFrame) || !outRender || !outMasks || numCascades > 16) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const size_t words = ((size_t)numEntities + 63) / 64;
    uint32_t added[16];                       // bCascadeAdded[z]: the shadow type of a cascade that is rendered this frame, 0 = None
    uint32_t snapshotIndex = firstSnapshot;
    for (uint32_t k = 0; k < numCascades; k++) {
        added[k] = 0u;
        uint64_t* m = outMasks + (size_t)k * words;
        std::memcpy(m, overlapMasks + (size_t)k * words, words * 8);
        for (uint32_t z = 0; z < k; z++)       // :310-327 "don't duplicate data for higher cascades"
            if (added[z] != 0u && added[z] == shadowTypes[k])
                for (size_t w = 0; w < words; w++) m[w] &= ~overlapMasks[(size_t)z * words + w];
        CsmLightState snap;                    // :334-347
        snap.hasView = view != nullptr;
        if (view) snap.view = *view;
        for (uint32_t i = 0; i < numEntities; i++)
            if ((m[i >> 6] >> (i & 63)) & 1ull) { snap.meshes.push_back(i); snap.frames.push_back(lastChangedFrame[i]); }
        bool same = false;
        if (snapshotIndex < state->states.size()) {
            const CsmLightState& old = state->states[snapshotIndex];
            same = old.meshes == snap.meshes && old.frames == snap.frames;
            if (same && (snap.hasView || old.hasView)) same = view_unchanged(old.hasView, old.view, snap.hasView, snap.view);
            if (!same) state->states[snapshotIndex] = std::move(snap); // :358
        } else {
            state->states.resize(snapshotIndex);  // (a gap can only come from a caller that skips indices: filled with empty states)
            state->states.push_back(std::move(snap)); // :363
        }
        outRender[k] = same ? 0u : 1u;         // an equal snapshot is kept as it is, camera included (:353-357)
        if (!same) added[k] = shadowTypes[k];
        snapshotIndex++;
    }
    return SAILOR_HIP_OK;
}

// ImGui_SetupRenderState (Submodules/ImGuiApi.cpp:118-125) and ImGui_RenderDrawData's loop (:197-275), over ImDrawData as plain data.  fp32 throughout;
// the casts are the reference's: (int) of a product for the size, (int32_t) of the clamped ends and of their DIFFERENCE for the scissor.
int sailor_host_ui_flatten(const float* displayPos, const float* displaySize, const float* framebufferScale, const SailorUiDrawList* lists, uint32_t numLists,
                           const SailorUiDrawCmd* cmds, uint32_t numCmds, float* outPushConstants, SailorUiCommand* outCommands, uint32_t maxCommands,
                           uint32_t* outNumCommands, int32_t* outWidth, int32_t* outHeight)
{
    if (!displayPos || !displaySize || !framebufferScale || (numLists && !lists) || (numCmds && !cmds) || !outPushConstants || !outNumCommands)
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    *outNumCommands = 0;
    // (a product that does not fit an int -- NaN, beyond 2^31 -- has no defined cast: refused)
    const float fw = displaySize[0] * framebufferScale[0], fh = displaySize[1] * framebufferScale[1];
    if (!(fw > -2147483648.0f && fw < 2147483648.0f) || !(fh > -2147483648.0f && fh < 2147483648.0f)) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const int width = (int)fw, height = (int)fh; // :198-199
    if (outWidth) *outWidth = width;
    if (outHeight) *outHeight = height;
    outPushConstants[0] = 2.0f / displaySize[0]; // :119-123
    outPushConstants[1] = 2.0f / displaySize[1];
    outPushConstants[2] = -1.0f - displayPos[0] * outPushConstants[0];
    outPushConstants[3] = -1.0f - displayPos[1] * outPushConstants[1];
    if (width <= 0 || height <= 0) return SAILOR_HIP_OK; // :201-202
    for (uint32_t n = 0; n < numLists; n++)
        if ((uint64_t)lists[n].firstCmd + lists[n].cmdCount > numCmds) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    uint64_t globalVtxOffset = 0, globalIdxOffset = 0;
    uint32_t count = 0;
    for (uint32_t n = 0; n < numLists; n++) {
        for (uint32_t i = 0; i < lists[n].cmdCount; i++) {
            const SailorUiDrawCmd& pcmd = cmds[lists[n].firstCmd + i];
            if (pcmd.callback != SAILOR_UI_CALLBACK_NONE) continue; // :224-232: a reset re-issues the state this flat form carries once, a user callback draws nothing
            float minX = (pcmd.clipRect[0] - displayPos[0]) * framebufferScale[0], minY = (pcmd.clipRect[1] - displayPos[1]) * framebufferScale[1]; // :236-237
            float maxX = (pcmd.clipRect[2] - displayPos[0]) * framebufferScale[0], maxY = (pcmd.clipRect[3] - displayPos[1]) * framebufferScale[1];
            if (minX < 0.0f) minX = 0.0f; // :240-243
            if (minY < 0.0f) minY = 0.0f;
            if (maxX > (float)width) maxX = (float)width;
            if (maxY > (float)height) maxY = (float)height;
            if (maxX <= minX || maxY <= minY) continue; // :244-245
            if (!(maxX > minX) || !(maxY > minY)) continue; // (a NaN ClipRect fails :244's test and would reach an undefined cast: left out)
            const uint64_t first = (uint64_t)pcmd.idxOffset + globalIdxOffset, vertex = (uint64_t)pcmd.vtxOffset + globalVtxOffset;
            if (first > 0xFFFFFFFFull || vertex > 0x7FFFFFFFull) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
            if (outCommands && count < maxCommands) {
                SailorUiCommand& c = outCommands[count];
                c.firstIndex = (uint32_t)first; c.indexCount = pcmd.elemCount; c.vertexOffset = (int32_t)vertex; // :265-270
                c.scissor[0] = (int32_t)minX; c.scissor[1] = (int32_t)minY;                                      // :250
                c.scissor[2] = (int32_t)(maxX - minX); c.scissor[3] = (int32_t)(maxY - minY);                    // :251
            }
            count++;
        }
        globalIdxOffset += lists[n].idxCount; // :273-274
        globalVtxOffset += lists[n].vtxCount;
    }
    *outNumCommands = count;
    return SAILOR_HIP_OK;
}

} // extern "C"
