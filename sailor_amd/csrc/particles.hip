// ExperimentalParticles (FrameGraph/ParticlesNode.cpp:184-257): the update of the per-instance SSBO, the node's order-resolved shadow map and the lit
// draw into Main / DepthBuffer.  include/sailor_hip.h has the pinned rules; tests/particles_ref.py restates the three stages in float64 and in fp32.
//
//   k_particles_update      ComputeParticles.shader:85-137, a lane per instance: two 80-byte records in as five float4 each (a record index at or past
//                           numRecords is the zero record, nothing is fetched), 96 bytes out as six float4 and isCulled as one dword; materialInstance and
//                           the padding are not touched.
//   k_particles_seed        one 64-bit key per texel: 0 (the map) or depth bits << 32 (the frame)
//   k_particles_cast        Particle.shader:125 under SHADOW_CASTER: a lane per (instance, triangle); clip = (lightsMatrices[0] * model) * p, then
//                           raster.hip's rules through surface_setup and surf_fill.  There is no depth attachment, so the key is (order + 1) << 32 | depth
//                           bits: the unsigned maximum keeps the LAST primitive of Vulkan's primitive order, whatever its depth.
//   k_particles_store_map   map = the key's low word; an untouched texel is 0, the clear value
//   k_particles_visibility  Particle.shader:122: the surface pass's key, depth bits << 32 | (order + 1), GreaterOrEqual in primitive order
//   k_particles_resolve     a lane per pixel: key -> instance, triangle, part; the set-up again, the varyings (:119-135) perspective-correct at the pixel, the
//                           fragment stage (:246-252) with shade_body.h's shadow_pcf over the R32 map; Main and DepthBuffer are written where a particle
//                           primitive owns the pixel and nowhere else.
// Light record 0 and matrix 0 are read by the kernels from the buffers the lights path fills (wave-uniform addresses: scalar loads).
//
// GLSL forms (sky.hip's header lists them): dot = (xx + yy) + zz, length = sqrt(dot(v, v)), normalize = v / length, distance = length(a - b), IEEE division and
// square root, mix(x, y, a) = x * (1 - a) + y * a, mod(x, y) = x - y * floor(x / y); sinf, cosf, acosf and powf are the device library's, as in ibl_prefilter.hip.
#include "surface_fill.h"
#include "shade_body.h"

#define PART_RECORD4 5u      // float4 per SailorParticleData
#define PART_INSTANCE4 7u    // float4 per SailorParticleInstance
#define PART_INSTANCE_FLOATS 28

// uint(f) as v_cvt_u32_f32 defines it: NaN and negatives -> 0, saturating at 2^32 - 1
__device__ __forceinline__ uint32_t part_cvt_u32(float x)
{
    if (!(x > 0.0f)) return 0u;
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)x;
}
__device__ __forceinline__ float part_mod(float x, float y) { return x - y * floorf(x / y); }

// a * b, both column-major: column j = a * b[j] (GLSL)
__device__ __forceinline__ Mat4 part_mul(const Mat4& a, const Mat4& b)
{
    Mat4 o;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float4 c = glsl_mul(a, b.m[4 * j + 0], b.m[4 * j + 1], b.m[4 * j + 2], b.m[4 * j + 3]);
        o.m[4 * j + 0] = c.x; o.m[4 * j + 1] = c.y; o.m[4 * j + 2] = c.z; o.m[4 * j + 3] = c.w;
    }
    return o;
}
__device__ __forceinline__ Mat4 part_identity()
{
    Mat4 o;
#pragma unroll
    for (int q = 0; q < 16; q++) o.m[q] = (q % 5 == 0) ? 1.0f : 0.0f;
    return o;
}

struct PartRecord { float4 q[5]; };
__device__ __forceinline__ PartRecord part_record(const float4* __restrict__ records, uint32_t numRecords, uint32_t index)
{
    PartRecord r;
    if (index < numRecords) {
#pragma unroll
        for (int k = 0; k < 5; k++) r.q[k] = records[(size_t)index * PART_RECORD4 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 5; k++) r.q[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return r;
}

__global__ __launch_bounds__(256) void k_particles_update(SailorParticlesConstants pc, float currentTime, const float4* __restrict__ records, uint32_t numRecords,
                                                          float4* __restrict__ instances)
{
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= pc.numInstances) return;
    // :100-102
    const uint32_t frame = part_cvt_u32(part_mod(currentTime * (float)pc.fps, (float)pc.numFrames));
    const uint32_t current = part_cvt_u32(part_mod((float)id, (float)pc.traceFrames));
    const float decay = powf(pc.traceDecay, (float)current);
    // :106-107, 32-bit unsigned and wrapping; max(0, .) is max(uint, uint) and clamps nothing
    const uint32_t tail = id / pc.traceFrames;
    const uint32_t iNew = (frame - current) * pc.numInstances / pc.traceFrames + tail;
    const uint32_t iOld = (frame - current - 1u) * pc.numInstances / pc.traceFrames + tail;
    const PartRecord n = part_record(records, numRecords, iNew), o = part_record(records, numRecords, iOld);
    const float enabled = n.q[0].x, size2 = n.q[0].z;
    const float x1 = n.q[1].x, y1 = n.q[1].y, z1 = n.q[1].z, x2 = n.q[3].x, y2 = n.q[3].y, z2 = n.q[3].z;
    // :110-111
    const float ex = x2 - x1, ey = y2 - y1, ez = z2 - z1;
    const float dist = sqrtf(dot3f(ex, ey, ez, ex, ey, ez));
    const float dx = ex / dist, dy = ey / dist, dz = ez / dist;
    // :113-115, up = (0, 0, 1)
    const float ax = 0.0f * dz - dy * 1.0f, ay = 1.0f * dx - dz * 0.0f, az = 0.0f * dy - dx * 0.0f;
    const float angle = acosf((0.0f * dx + 0.0f * dy) + 1.0f * dz);
    Mat4 R = part_identity();
    const float alen = sqrtf(dot3f(ax, ay, az, ax, ay, az));
    if (alen > 0.0f) { // :118; :60-82
        const float c = cosf(angle), s = sinf(angle), omc = 1.0f - c;
        const float ux = ax / alen, uy = ay / alen, uz = az / alen;
        R.m[0] = c + ux * ux * omc;      R.m[1] = ux * uy * omc - uz * s; R.m[2] = ux * uz * omc + uy * s;
        R.m[4] = uy * ux * omc + uz * s; R.m[5] = c + uy * uy * omc;      R.m[6] = uy * uz * omc - ux * s;
        R.m[8] = uz * ux * omc - uy * s; R.m[9] = uz * uy * omc + ux * s; R.m[10] = c + uz * uz * omc;
    }
    // :123-133
    Mat4 S = part_identity();
    S.m[10] = dist;
    S.m[0] = S.m[5] = size2 * decay * 1.5f;
    Mat4 T = part_identity();
    T.m[12] = (x1 + x2) * 0.5f; T.m[13] = (y1 + y2) * 0.5f; T.m[14] = (z1 + z2) * 0.5f; T.m[15] = 1.0f;
    const Mat4 M = part_mul(part_mul(T, R), S);
    float4* out = instances + (size_t)id * PART_INSTANCE4;
    out[0] = make_float4(M.m[0], M.m[1], M.m[2], M.m[3]);
    out[1] = make_float4(M.m[4], M.m[5], M.m[6], M.m[7]);
    out[2] = make_float4(M.m[8], M.m[9], M.m[10], M.m[11]);
    out[3] = make_float4(M.m[12], M.m[13], M.m[14], M.m[15]);
    out[4] = make_float4(n.q[4].x, n.q[4].y, n.q[4].z, n.q[4].w * decay); // :135 color
    out[5] = make_float4(o.q[4].x, o.q[4].y, o.q[4].z, o.q[4].w * decay); // :134 colorOld
    reinterpret_cast<uint32_t*>(out)[25] = enabled > 0.5f ? 1u : 0u;      // :136 isCulled
}

// ---- the two passes ---------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_particles_seed(const float* __restrict__ depth, size_t texels, unsigned long long* __restrict__ keys)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < texels) keys[g] = depth ? (unsigned long long)__float_as_uint(depth[g]) << 32 : 0ull;
}

// MAP: clip = (lightsMatrices[0] * model) * p and the order in the key's high word; else clip = projection * (view * (model * p)) and the surface pass's key.
// The gridDim.y slices are k_surface_visibility's.
template <bool MAP>
__global__ __launch_bounds__(256) void k_particles_raster(Mat4 P, Mat4 V, const float* __restrict__ lightsMatrices, SailorParticlesDraw draw,
                                                          const float* __restrict__ instances, uint32_t numInstances, int W, int H,
                                                          unsigned long long* __restrict__ keys)
{
    const float* __restrict__ vertices = reinterpret_cast<const float*>(draw.dVertices);
    const unsigned long long total = (unsigned long long)numInstances * draw.numTriangles;
    const unsigned long long id = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool have = id < total;
    uint32_t inst = 0, tri = 0;
    if (have) { inst = (uint32_t)(id / draw.numTriangles); tri = (uint32_t)(id - (unsigned long long)inst * draw.numTriangles); }
    const float* __restrict__ model = instances + PART_INSTANCE_FLOATS * (size_t)inst;
    Mat4 LM = part_identity();
    if (MAP && have) {
        Mat4 L, M;
#pragma unroll
        for (int q = 0; q < 16; q++) { L.m[q] = lightsMatrices[q]; M.m[q] = model[q]; }
        LM = part_mul(L, M);
    }
    bool again = false;
    for (int part = 0; part < 2; part++) {
        if (part && !__any(again)) break;
        SurfTri t;
        t.valid = false;
        bool second = false;
        if (have && (part == 0 || again)) {
            SurfSrc S;
            if (MAP) t = surface_setup_matrix(LM, vertices, draw.dIndices + 3 * (size_t)tri, W, H, 0, H, true, part, second, S);
            else t = surface_setup(P, V, model, vertices, draw.dIndices + 3 * (size_t)tri, W, H, 0, H, true, part, second, S);
        }
        const unsigned int orderPlus1 = (unsigned int)(2ull * id) + (unsigned int)part + 1u; // (the entry point has checked the range)
        surf_fill(t, orderPlus1, SurfNoPayload(), SurfNoBcast(), blockIdx.y, gridDim.y, lane, [&](int i, int j, float z, unsigned int tag, auto&&...) {
            unsigned long long* p = keys + (size_t)j * W + i;
            if (MAP) {
                const unsigned long long key = ((unsigned long long)tag << 32) | __float_as_uint(z);
                if (key > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, key);
            } else surf_fragment(p, z, tag);
        });
        if (part == 0) again = second;
    }
}

__global__ __launch_bounds__(256) void k_particles_store_map(const unsigned long long* __restrict__ keys, size_t texels, float* __restrict__ map)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < texels) map[g] = __uint_as_float((unsigned int)keys[g]);
}

// varying c of source vertex v under instance m (Particle.shader:119-135): 0-2 worldPosition, 3-6 color = mix(color, colorOld, (p.z + 1) / 2),
// 7-9 mat3(model) * inNormal, the third column of tangentBasis
__device__ __forceinline__ float part_varying(const float* __restrict__ v, const float* __restrict__ m, int c)
{
    const float x = v[2], y = v[3], z = v[4];
    if (c < 3) {
        const float a = ((m[c] * x + m[4 + c] * y) + m[8 + c] * z) + m[12 + c] * 1.0f;
        const float w = ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * 1.0f;
        return a / w;
    }
    if (c < 7) {
        const float a = (z + 1.0f) / 2.0f;
        return m[16 + (c - 3)] * (1.0f - a) + m[20 + (c - 3)] * a;
    }
    const int r = c - 7;
    return (m[r] * v[5] + m[4 + r] * v[6]) + m[8 + r] * v[7];
}

__global__ __launch_bounds__(256) void k_particles_resolve(Mat4 P, Mat4 V, SailorParticlesDraw draw, const float* __restrict__ instances, uint32_t numInstances,
                                                           const float* __restrict__ lights, const float* __restrict__ lightsMatrices,
                                                           const float* __restrict__ map, int mapW, int mapH, float texelW, float texelH,
                                                           const unsigned long long* __restrict__ keys, float4* __restrict__ target, float* __restrict__ depth,
                                                           int W, int H)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const size_t at = (size_t)j * W + i;
    const unsigned long long key = keys[at];
    const unsigned int low = (unsigned int)key;
    if (low == 0u) return; // no particle primitive owns the pixel: both targets stay as they are
    const unsigned int order = low - 1u, per = 2u * draw.numTriangles;
    const unsigned int inst = order / per, r = order - inst * per, tri = r >> 1;
    if (inst >= numInstances) return;
    const float* __restrict__ model = instances + PART_INSTANCE_FLOATS * (size_t)inst;
    const float* __restrict__ vertices = reinterpret_cast<const float*>(draw.dVertices);
    bool second;
    SurfSrc S;
    const SurfTri t = surface_setup(P, V, model, vertices, draw.dIndices + 3 * (size_t)tri, W, H, 0, H, true, (int)(r & 1u), second, S);
    if (!t.valid) return;
    const long long px = 256ll * i + 128, py = 256ll * j + 128;
    const float area = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
    const float l0 = (float)surf_edge(t.x1, t.y1, t.x2, t.y2, px, py) / area, l1 = (float)surf_edge(t.x2, t.y2, t.x0, t.y0, px, py) / area,
                l2 = (float)surf_edge(t.x0, t.y0, t.x1, t.y1, px, py) / area;
    const float q0 = l0 / S.w[0], q1 = l1 / S.w[1], q2 = l2 / S.w[2];
    const float s = (q0 + q1) + q2;
    const float b0 = q0 / s, b1 = q1 / s, b2 = q2 / s;
    const float* __restrict__ vI0 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[0];
    const float* __restrict__ vI1 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[1];
    const float* __restrict__ vI2 = vertices + SURF_VERTEX_FLOATS * (size_t)S.I[2];
    const float* __restrict__ vO1 = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[1];
    const float* __restrict__ vO2 = vertices + SURF_VERTEX_FLOATS * (size_t)S.O[2];
    float a[10];
#pragma unroll
    for (int c = 0; c < 10; c++) {
        const float a0 = part_varying(vI0, model, c); // (vertex 0 is never a cut one)
        float a1 = part_varying(vI1, model, c), a2 = part_varying(vI2, model, c);
        if (S.cut[1]) a1 = a1 + (part_varying(vO1, model, c) - a1) * S.t[1];
        if (S.cut[2]) a2 = a2 + (part_varying(vO2, model, c) - a2) * S.t[2];
        a[c] = (a0 * b0 + a1 * b1) + a2 * b2;
    }
    // :249-252
    const float nlen = sqrtf(dot3f(a[7], a[8], a[9], a[7], a[8], a[9]));
    const float nx = a[7] / nlen, ny = a[8] / nlen, nz = a[9] / nlen;
    const float lighting = glsl_max(0.0f, dot3f(-lights[8], -lights[9], -lights[10], nx, ny, nz)); // SailorLightShaderData.direction of record 0
    Mat4 L;
#pragma unroll
    for (int q = 0; q < 16; q++) L.m[q] = lightsMatrices[q];
    const float4 lp = glsl_mul(L, a[0], a[1], a[2], 1.0f);
    const float shadow = shadow_pcf(map, SAILOR_SHADOWMAP_R32_SFLOAT, mapW, mapH, texelW, texelH, lp, 0.00001f);
    const float f = glsl_max(0.05f, glsl_min(lighting, shadow));
    target[at] = make_float4(a[3] * f, a[4] * f, a[5] * f, a[6]);
    depth[at] = __uint_as_float((unsigned int)(key >> 32));
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------------------------

static int part_refuse(SailorHipContext* ctx, const char* what)
{
    ctx->lastError = what;
    return SAILOR_HIP_ERR_INVALID_ARGUMENT;
}
static bool part_finite(float x) { return x - x == 0.0f; }

// what both passes check of the draw and the instances; NULL = fine
static const char* part_draw_refusal(const SailorParticlesDraw* draw, const SailorParticleInstance* dInstances, uint32_t numInstances)
{
    if (!draw) return "the draw is NULL";
    if (!aligned(draw->dVertices, 4) || !aligned(draw->dIndices, 4)) return "the vertex or index buffer is NULL or misaligned";
    if (!aligned(dInstances, 16)) return "the instance buffer is NULL or not 16-byte aligned";
    if (numInstances == 0 || draw->numTriangles == 0) return "numInstances or numTriangles is 0";
    if ((unsigned long long)numInstances * 2ull * draw->numTriangles >= 0xFFFFFFFFull) return "numInstances * 2 * numTriangles reaches 2^32 - 1";
    return nullptr;
}
static dim3 part_raster_grid(uint32_t numInstances, uint32_t numTriangles)
{
    const unsigned long long total = (unsigned long long)numInstances * numTriangles; // (< 2^31: see part_draw_refusal)
    return dim3((unsigned)((total + 255) / 256), surf_slices(total));
}

extern "C" {

int sailor_hip_particles_update(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorParticlesConstants* constants, const SailorParticleData* dRecords,
                                uint32_t numRecords, SailorParticleInstance* dInstances)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!frame || !constants) return part_refuse(ctx, "sailor_hip_particles_update: frame or constants is NULL");
    if (!aligned(dRecords, 16) || !aligned(dInstances, 16)) return part_refuse(ctx, "sailor_hip_particles_update: records or instances NULL or not 16-byte aligned");
    const SailorParticlesConstants pc = *constants;
    if (pc.numInstances == 0 || pc.numInstances > 0x7FFFFFFFu) return part_refuse(ctx, "sailor_hip_particles_update: numInstances is 0 or above 2^31 - 1");
    if (pc.traceFrames == 0 || pc.numFrames == 0) return part_refuse(ctx, "sailor_hip_particles_update: traceFrames or numFrames is 0 (the shader divides by them)");
    if (!part_finite(pc.traceDecay) || !(pc.traceDecay > 0.0f)) return part_refuse(ctx, "sailor_hip_particles_update: traceDecay is not finite or not > 0");
    const float t = frame->currentTime * (float)pc.fps;
    if (!part_finite(t) || t < 0.0f) return part_refuse(ctx, "sailor_hip_particles_update: currentTime * fps is not finite or negative");
    if (overlaps(dRecords, (size_t)numRecords * sizeof(SailorParticleData), dInstances, (size_t)pc.numInstances * sizeof(SailorParticleInstance)))
        return part_refuse(ctx, "sailor_hip_particles_update: records and instances overlap");
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    sailor_launch(ctx, k_particles_update, dim3((pc.numInstances + 255u) / 256u), dim3(256), pc, frame->currentTime, reinterpret_cast<const float4*>(dRecords), numRecords,
                  reinterpret_cast<float4*>(dInstances));
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_update");
    return SAILOR_HIP_OK;
}

size_t sailor_hip_particles_workspace_bytes(int32_t mapWidth, int32_t mapHeight, int32_t width, int32_t height)
{
    if (!extent_ok(mapWidth, mapHeight) || !extent_ok(width, height)) return 0;
    const size_t a = (size_t)mapWidth * mapHeight, b = (size_t)width * height;
    return align_up(8 * (a > b ? a : b), 256);
}

int sailor_hip_particles_shadow(SailorHipContext* ctx, const SailorParticlesDraw* draw, const SailorParticleInstance* dInstances, uint32_t numInstances,
                                const float* dLightsMatrices, float* dShadowMap, int32_t mapWidth, int32_t mapHeight, void* dWorkspace, size_t workspaceBytes)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (const char* why = part_draw_refusal(draw, dInstances, numInstances)) { ctx->lastError = std::string("sailor_hip_particles_shadow: ") + why; return SAILOR_HIP_ERR_INVALID_ARGUMENT; }
    if (!extent_ok(mapWidth, mapHeight)) return part_refuse(ctx, "sailor_hip_particles_shadow: the map's extent is outside 1 .. 32768");
    if (!aligned(dLightsMatrices, 16) || !aligned(dShadowMap, 4) || !aligned(dWorkspace, 16))
        return part_refuse(ctx, "sailor_hip_particles_shadow: matrices, map or workspace NULL or misaligned");
    const size_t texels = (size_t)mapWidth * mapHeight, instBytes = (size_t)numInstances * sizeof(SailorParticleInstance);
    if (workspaceBytes < 8 * texels) return part_refuse(ctx, "sailor_hip_particles_shadow: the workspace is too small");
    if (overlaps(dShadowMap, 4 * texels, dInstances, instBytes) || overlaps(dShadowMap, 4 * texels, dWorkspace, workspaceBytes) ||
        overlaps(dWorkspace, workspaceBytes, dInstances, instBytes) || overlaps(dShadowMap, 4 * texels, dLightsMatrices, 64) || overlaps(dWorkspace, workspaceBytes, dLightsMatrices, 64))
        return part_refuse(ctx, "sailor_hip_particles_shadow: the map, the workspace and the inputs overlap");
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(dWorkspace);
    const unsigned texelBlocks = (unsigned)((texels + 255) / 256);
    sailor_launch(ctx, k_particles_seed, dim3(texelBlocks), dim3(256), (const float*)nullptr, texels, keys);
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_seed");
    Mat4 none {};
    sailor_launch(ctx, k_particles_raster<true>, part_raster_grid(numInstances, draw->numTriangles), dim3(256), none, none, dLightsMatrices, *draw,
                  reinterpret_cast<const float*>(dInstances), numInstances, (int)mapWidth, (int)mapHeight, keys);
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_cast");
    sailor_launch(ctx, k_particles_store_map, dim3(texelBlocks), dim3(256), (const unsigned long long*)keys, texels, dShadowMap);
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_store_map");
    return SAILOR_HIP_OK;
}

int sailor_hip_particles_draw(SailorHipContext* ctx, const SailorUboFrameData* frame, const SailorParticlesDraw* draw, const SailorParticleInstance* dInstances,
                              uint32_t numInstances, const SailorLightShaderData* dLights, const float* dLightsMatrices, const float* dShadowMap, int32_t mapWidth,
                              int32_t mapHeight, float* dMain, float* dDepth, int32_t width, int32_t height, void* dWorkspace, size_t workspaceBytes)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    if (!frame) return part_refuse(ctx, "sailor_hip_particles_draw: frame is NULL");
    if (const char* why = part_draw_refusal(draw, dInstances, numInstances)) { ctx->lastError = std::string("sailor_hip_particles_draw: ") + why; return SAILOR_HIP_ERR_INVALID_ARGUMENT; }
    if (!extent_ok(mapWidth, mapHeight) || !extent_ok(width, height)) return part_refuse(ctx, "sailor_hip_particles_draw: an extent is outside 1 .. 32768");
    if (!aligned(dLights, 16) || !aligned(dLightsMatrices, 16) || !aligned(dShadowMap, 4) || !aligned(dMain, 16) || !aligned(dDepth, 4) || !aligned(dWorkspace, 16))
        return part_refuse(ctx, "sailor_hip_particles_draw: a buffer is NULL or misaligned");
    const size_t pixels = (size_t)width * height, texels = (size_t)mapWidth * mapHeight, instBytes = (size_t)numInstances * sizeof(SailorParticleInstance);
    if (workspaceBytes < 8 * pixels) return part_refuse(ctx, "sailor_hip_particles_draw: the workspace is too small");
    const void* in[] = { dInstances, dLights, dLightsMatrices, dShadowMap };
    const size_t inBytes[] = { instBytes, sizeof(SailorLightShaderData), 64, 4 * texels };
    for (int k = 0; k < 4; k++)
        if (overlaps(dMain, 16 * pixels, in[k], inBytes[k]) || overlaps(dDepth, 4 * pixels, in[k], inBytes[k]) || overlaps(dWorkspace, workspaceBytes, in[k], inBytes[k]))
            return part_refuse(ctx, "sailor_hip_particles_draw: an output or the workspace overlaps an input");
    if (overlaps(dMain, 16 * pixels, dDepth, 4 * pixels) || overlaps(dMain, 16 * pixels, dWorkspace, workspaceBytes) || overlaps(dDepth, 4 * pixels, dWorkspace, workspaceBytes))
        return part_refuse(ctx, "sailor_hip_particles_draw: Main, DepthBuffer and the workspace overlap");
    Mat4 P, V;
    memcpy(P.m, frame->projection, 64);
    memcpy(V.m, frame->view, 64);
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(dWorkspace);
    sailor_launch(ctx, k_particles_seed, dim3((unsigned)((pixels + 255) / 256)), dim3(256), (const float*)dDepth, pixels, keys);
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_seed");
    sailor_launch(ctx, k_particles_raster<false>, part_raster_grid(numInstances, draw->numTriangles), dim3(256), P, V, dLightsMatrices, *draw,
                  reinterpret_cast<const float*>(dInstances), numInstances, (int)width, (int)height, keys);
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_visibility");
    sailor_launch(ctx, k_particles_resolve, texel_grid(width, height), dim3(256), P, V, *draw, reinterpret_cast<const float*>(dInstances), numInstances,
                  reinterpret_cast<const float*>(dLights), dLightsMatrices, dShadowMap, (int)mapWidth, (int)mapHeight, 1.0f / (float)mapWidth, 1.0f / (float)mapHeight,
                  (const unsigned long long*)keys, reinterpret_cast<float4*>(dMain), dDepth, (int)width, (int)height);
    SAILOR_CHECK_LAUNCH(ctx, "k_particles_resolve");
    return SAILOR_HIP_OK;
}

} // extern "C"
