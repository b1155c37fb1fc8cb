// A stand-alone program over the host-side logic the glTF materials added: every refusal of sailor_hip_surface_draw_gltf, sailor_hip_surface_resolve_gltf and
// sailor_hip_surface_composite_gltf (argument checks, flag bits, the tables ALPHA_CUTOUT requires, alignment, the workspace's size arithmetic), the record's
// layout, and the harness's shader list (sailor_amd/runtime/scene_tags.h), built with the sanitizers on the host side.  No GPU is needed or used: every call
// here is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/gltf_host_check.cpp -o /tmp/gltf_host_check -L. -lsailor_hip -Wl,-rpath,$PWD && /tmp/gltf_host_check
#include "../sailor_amd/csrc/surface_gltf.hip"
#include "../sailor_amd/runtime/scene_tags.h"
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool refused(SailorHipContext& ctx, int status, const char* text)
{
    const bool ok = status == SAILOR_HIP_ERR_INVALID_ARGUMENT && ctx.launchCount == 0 && ctx.lastError.find(text) != std::string::npos;
    if (!ok) printf("  status %d, launches %llu, last_error '%s', wanted '%s'\n", status, (unsigned long long)ctx.launchCount, ctx.lastError.c_str(), text);
    ctx.lastError.clear();
    return ok;
}

int main()
{
    // Standard_glTF.shader:42-58 under std430, in SailorMaterialData's stride: the table is one array
    static_assert(sizeof(SailorGltfMaterialData) == 80 && sizeof(SailorGltfMaterialData) == sizeof(SailorMaterialData), "one table of 80-byte slots");
    static_assert(offsetof(SailorGltfMaterialData, emissiveFactor) == 16 && offsetof(SailorGltfMaterialData, metallicFactor) == 32 &&
                  offsetof(SailorGltfMaterialData, alphaCutoff) == 48 && offsetof(SailorGltfMaterialData, baseColorSampler) == 52 &&
                  offsetof(SailorGltfMaterialData, emissiveSampler) == 68, "std430 offsets");
    SailorHipContext ctx;
    const int32_t W = 40, H = 24;
    SailorBand band, bad;
    sailor_hip_band_whole_frame(W, H, &band);
    bad = band; bad.fbRowCount = H + 1;
    const size_t bytes = sailor_hip_surface_workspace_bytes(W, H, &band, 2);
    // device pointers are never dereferenced on the host: aligned fakes
    alignas(16) static char fake[64];
    void* ws = fake;
    const auto* inst = reinterpret_cast<const SailorPerInstanceData*>(fake);
    const auto* mats = reinterpret_cast<const SailorMaterialData*>(fake);
    const auto* tex = reinterpret_cast<const SailorTextureDesc*>(fake);
    float* plane = reinterpret_cast<float*>(fake);
    float* odd4 = reinterpret_cast<float*>(fake + 4);   // 4-byte aligned, not 16
    float* odd2 = reinterpret_cast<float*>(fake + 2);
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 1; d.flags = SAILOR_SURFACE_GLTF | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK;
    auto draw = [&](const SailorSurfaceDraw* dd, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt, uint32_t index,
                    const SailorBand* b, void* w, size_t n) { return sailor_hip_surface_draw_gltf(&ctx, &frame, dd, i, m, nm, t, nt, index, W, H, b, w, n); };
    EXPECT(sailor_hip_surface_draw_gltf(nullptr, &frame, &d, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_draw_gltf(&ctx, nullptr, &d, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "frame or draw is NULL"));
    EXPECT(refused(ctx, draw(nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "frame or draw is NULL"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &bad, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, nullptr, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes), "workspace is NULL"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes), "not 16-byte aligned"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, ws, 0), "too small"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 2, &band, ws, bytes), "drawIndex"));
    EXPECT(refused(ctx, draw(&d, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 0, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, nullptr, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 0, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes), "buffer is NULL"));
    for (uint32_t bit = 3; bit < 32; bit++) {
        SailorSurfaceDraw e = d;
        e.flags = d.flags | (1u << bit);
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "unknown flags"));
    }
    for (uint32_t flags = 0; flags < 4; flags++) { // every combination without the glTF bit
        SailorSurfaceDraw e = d;
        e.flags = flags;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "does not carry SAILOR_SURFACE_GLTF"));
    }
    {
        SailorSurfaceDraw e = d;
        e.primBase = 0xFFFFFFFFu - 4u;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.numTriangles = 0xFFFFFFFFu; e.numDrawn = 0xFFFFFFFFu;   // the product needs 64 bits
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        // the two older draw calls keep refusing the bit
        e = d;
        EXPECT(sailor_hip_surface_draw_masked(&ctx, &frame, &e, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT &&
               ctx.launchCount == 0 && ctx.lastError.find("sailor_hip_surface_draw_masked: unknown flags") != std::string::npos);
    }
    auto resolve = [&](const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt, const SailorBand* b, const void* w,
                       size_t n, float* surface, size_t stride, float* depth, const float* aoIn, float* aoOut, float* emissive) {
        return sailor_hip_surface_resolve_gltf(&ctx, &frame, i, m, nm, t, nt, W, H, b, w, n, surface, stride, depth, nullptr, aoIn, aoOut, emissive);
    };
    const size_t px = (size_t)W * H;
    EXPECT(sailor_hip_surface_resolve_gltf(nullptr, &frame, inst, mats, 1, tex, 1, W, H, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, nullptr, plane) ==
           SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, resolve(nullptr, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(inst, nullptr, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(inst, mats, 0, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, nullptr, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 0, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &bad, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "band is not valid"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, nullptr, bytes, plane, px, nullptr, nullptr, nullptr, plane), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, 64 + 1024 + px * 8, plane, px, nullptr, nullptr, nullptr, plane), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, nullptr, px, nullptr, nullptr, nullptr, plane), "surface is NULL"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, odd4, px, nullptr, nullptr, nullptr, plane), "surface is NULL or not 16-byte aligned"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, plane, px - 1, nullptr, nullptr, nullptr, plane), "planeStride"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, odd2, nullptr, nullptr, plane), "depth output is misaligned"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, odd2, nullptr, plane), "occlusion plane is misaligned"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, odd2, plane), "occlusion plane is misaligned"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, nullptr), "emissive plane is NULL"));
    EXPECT(refused(ctx, resolve(inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, odd4), "emissive plane is NULL or not 16-byte aligned"));

    auto composite = [&](const float* rad, const float* em, const void* w, size_t n, float* target, const SailorBand* b) {
        return sailor_hip_surface_composite_gltf(&ctx, rad, em, w, n, target, W, H, b);
    };
    EXPECT(sailor_hip_surface_composite_gltf(nullptr, plane, plane, ws, bytes, plane, W, H, &band) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, composite(plane, plane, ws, bytes, plane, &bad), "band is not valid"));
    EXPECT(refused(ctx, composite(plane, plane, nullptr, bytes, plane, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, composite(plane, plane, ws, 100, plane, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, composite(nullptr, plane, ws, bytes, plane, &band), "radiance, emissive or target"));
    EXPECT(refused(ctx, composite(plane, nullptr, ws, bytes, plane, &band), "radiance, emissive or target"));
    EXPECT(refused(ctx, composite(plane, odd4, ws, bytes, plane, &band), "radiance, emissive or target"));
    EXPECT(refused(ctx, composite(plane, plane, ws, bytes, nullptr, &band), "radiance, emissive or target"));

    // ---- the harness's shader list ----
    const uint32_t good[4] = { 0, 1, 1, 0 }, two[2] = { 1, 2 }, high[1] = { 0x80000001u };
    EXPECT(sailor_rt_scene_shaders_ok(good, 4) && sailor_rt_scene_shaders_ok(good, 0) && sailor_rt_scene_shaders_ok(nullptr, 0));
    EXPECT(!sailor_rt_scene_shaders_ok(nullptr, 1) && !sailor_rt_scene_shaders_ok(two, 2) && sailor_rt_scene_shaders_ok(two, 1) && !sailor_rt_scene_shaders_ok(high, 1) &&
           !sailor_rt_scene_shaders_ok(good, -1));
    printf(failures ? "gltf_host_check: %d FAILED\n" : "gltf_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
