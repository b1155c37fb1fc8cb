// A stand-alone program over the host-side logic the Transparent queue added: every refusal of sailor_hip_surface_peel_begin, _peel_draw, _peel_draw_gltf,
// _peel_commit and sailor_hip_surface_blend (argument checks, the flag bits and the blend field, MULTIPLY's unsupported status, alignment, the workspace's
// size arithmetic), and that the older draw entries keep refusing the blend bits, built with the sanitizers on the host side.  No GPU is needed or used:
// every call here is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/transparent_host_check.cpp -o /tmp/transparent_host_check -L. -lsailor_hip -Wl,-rpath,$PWD \
//       && /tmp/transparent_host_check
#include "../sailor_amd/csrc/surface_transparent.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool refused(SailorHipContext& ctx, int status, const char* text, int want = SAILOR_HIP_ERR_INVALID_ARGUMENT)
{
    const bool ok = status == want && ctx.launchCount == 0 && ctx.lastError.find(text) != std::string::npos;
    if (!ok) printf("  status %d, launches %llu, last_error '%s', wanted '%s'\n", status, (unsigned long long)ctx.launchCount, ctx.lastError.c_str(), text);
    ctx.lastError.clear();
    return ok;
}

int main()
{
    static_assert(((SAILOR_SURFACE_BLEND_MASK << SAILOR_SURFACE_BLEND_SHIFT) & (SAILOR_SURFACE_CULL_BACK | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_GLTF)) == 0,
                  "the blend field lies above the existing flags");
    static_assert(SAILOR_SURFACE_BLEND_NONE == 0 && SAILOR_SURFACE_BLEND_ADDITIVE == 1 && SAILOR_SURFACE_BLEND_ALPHA == 2 && SAILOR_SURFACE_BLEND_MULTIPLY == 3, "EBlendMode");
    SailorHipContext ctx;
    const int32_t W = 50, H = 35;
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
    uint32_t* last = reinterpret_cast<uint32_t*>(fake);
    uint32_t* last2 = reinterpret_cast<uint32_t*>(fake + 2);
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 1;
    const uint32_t ALPHA = SAILOR_SURFACE_BLEND_ALPHA << SAILOR_SURFACE_BLEND_SHIFT, MULTIPLY = SAILOR_SURFACE_BLEND_MULTIPLY << SAILOR_SURFACE_BLEND_SHIFT;

    // ---- begin and commit ----
    EXPECT(sailor_hip_surface_peel_begin(nullptr, W, H, &band, ws, bytes, last, 1) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, &bad, ws, bytes, last, 1), "peel_begin: the band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, nullptr, ws, bytes, last, 1), "band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, 0, H, &band, ws, bytes, last, 1), "band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, &band, nullptr, bytes, last, 1), "workspace is NULL"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, &band, fake + 8, bytes, last, 1), "not 16-byte aligned"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, &band, ws, 64 + 1024 + (size_t)W * H * 8, last, 1), "too small"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, &band, ws, bytes, nullptr, 0), "last-order plane"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_begin(&ctx, W, H, &band, ws, bytes, last2, 0), "last-order plane"));
    EXPECT(sailor_hip_surface_peel_commit(nullptr, W, H, &band, ws, bytes, last, last) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &bad, ws, bytes, last, last), "peel_commit: the band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &band, nullptr, bytes, last, last), "workspace is NULL"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &band, ws, 100, last, last), "too small"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &band, ws, bytes, nullptr, last), "last-order plane"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &band, ws, bytes, last2, last), "last-order plane"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &band, ws, bytes, last, nullptr), "counter"));
    EXPECT(refused(ctx, sailor_hip_surface_peel_commit(&ctx, W, H, &band, ws, bytes, last, last2), "counter"));

    // ---- the two draws ----
    for (int g = 0; g < 2; g++) {
        const auto entry = g ? sailor_hip_surface_peel_draw_gltf : sailor_hip_surface_peel_draw;
        const char* who = g ? "sailor_hip_surface_peel_draw_gltf: " : "sailor_hip_surface_peel_draw: ";
        SailorSurfaceDraw base = d;
        base.flags = ALPHA | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK | (g ? SAILOR_SURFACE_GLTF : 0u);
        auto draw = [&](const SailorSurfaceDraw* dd, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt,
                        uint32_t index, const SailorBand* b, void* w, size_t n, const float* depth, const uint32_t* l) {
            return entry(&ctx, &frame, dd, i, m, nm, t, nt, index, W, H, b, w, n, depth, l);
        };
        EXPECT(entry(nullptr, &frame, &base, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes, plane, last) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(refused(ctx, entry(&ctx, nullptr, &base, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes, plane, last), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &bad, ws, bytes, plane, last), who));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &bad, ws, bytes, plane, last), "band is not valid"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes, plane, last), "workspace is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes, plane, last), "not 16-byte aligned"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, 0, plane, last), "too small"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 2, &band, ws, bytes, plane, last), "drawIndex"));
        EXPECT(refused(ctx, draw(&base, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes, plane, last), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 0, 0, &band, ws, bytes, plane, last), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&base, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last), "buffer is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, nullptr, last), "depth attachment"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, odd2, last), "depth attachment"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, nullptr), "last-order plane"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last2), "last-order plane"));
        for (uint32_t bit = 5; bit < 32; bit++) {
            SailorSurfaceDraw e = base;
            e.flags |= 1u << bit;
            EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last), "unknown flags"));
        }
        SailorSurfaceDraw e = base;
        e.flags = (base.flags & ~ALPHA) | MULTIPLY;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last), "Multiply", SAILOR_HIP_ERR_UNSUPPORTED));
        e = base; e.primBase = 0xFFFFFFFFu - 4u;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last), "reaches 2^32 - 1"));
        e = base; e.flags ^= SAILOR_SURFACE_GLTF;   // the glTF bit on the Standard entry, its absence on the glTF one
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, last), g ? "does not carry SAILOR_SURFACE_GLTF" : "unknown flags"));
    }

    // ---- the older draw entries keep refusing the blend bits ----
    for (uint32_t mode = 1; mode < 4; mode++) {
        SailorSurfaceDraw e = d;
        e.flags = mode << SAILOR_SURFACE_BLEND_SHIFT;
        EXPECT(refused(ctx, sailor_hip_surface_draw(&ctx, &frame, &e, inst, 0, W, H, &band, ws, bytes), "sailor_hip_surface_draw: unknown flags"));
        EXPECT(refused(ctx, sailor_hip_surface_draw_masked(&ctx, &frame, &e, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "sailor_hip_surface_draw_masked: unknown flags"));
        e.flags |= SAILOR_SURFACE_GLTF;
        EXPECT(refused(ctx, sailor_hip_surface_draw_gltf(&ctx, &frame, &e, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "sailor_hip_surface_draw_gltf: unknown flags"));
    }

    // ---- the blend ----
    auto blend = [&](const float* rad, const float* p0, const float* em, const void* w, size_t n, float* target, const SailorBand* b) {
        return sailor_hip_surface_blend(&ctx, rad, p0, em, w, n, target, W, H, b);
    };
    EXPECT(sailor_hip_surface_blend(nullptr, plane, plane, nullptr, ws, bytes, plane, W, H, &band) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, blend(plane, plane, nullptr, ws, bytes, plane, &bad), "sailor_hip_surface_blend: the band is not valid"));
    EXPECT(refused(ctx, blend(plane, plane, nullptr, nullptr, bytes, plane, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, blend(plane, plane, nullptr, ws, 100, plane, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, blend(nullptr, plane, nullptr, ws, bytes, plane, &band), "radiance, the surface's first plane or target"));
    EXPECT(refused(ctx, blend(plane, nullptr, nullptr, ws, bytes, plane, &band), "radiance, the surface's first plane or target"));
    EXPECT(refused(ctx, blend(plane, odd4, nullptr, ws, bytes, plane, &band), "radiance, the surface's first plane or target"));
    EXPECT(refused(ctx, blend(plane, plane, nullptr, ws, bytes, nullptr, &band), "radiance, the surface's first plane or target"));
    EXPECT(refused(ctx, blend(plane, plane, nullptr, ws, bytes, odd4, &band), "radiance, the surface's first plane or target"));
    EXPECT(refused(ctx, blend(plane, plane, odd4, ws, bytes, plane, &band), "emissive plane is not 16-byte aligned"));
    printf(failures ? "transparent_host_check: %d FAILED\n" : "transparent_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
