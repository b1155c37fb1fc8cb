// A stand-alone program over the host-side logic the Masked queue added: every refusal of sailor_hip_surface_draw_masked and sailor_hip_surface_store_depth
// (argument checks, flag bits, the tables the flag requires, the workspace's size arithmetic) and the harness's tag parsing (sailor_amd/runtime/scene_tags.h),
// built with the sanitizers on the host side.  No GPU is needed or used: every call here is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/masked_host_check.cpp -o /tmp/masked_host_check -L. -lsailor_hip -Wl,-rpath,$PWD && /tmp/masked_host_check
#include "../sailor_amd/csrc/surface_masked.hip"
#include "../sailor_amd/runtime/scene_tags.h"
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
    SailorHipContext ctx;
    const int32_t W = 40, H = 24;
    SailorBand band, bad;
    sailor_hip_band_whole_frame(W, H, &band);
    bad = band; bad.fbRowCount = H + 1;
    const size_t bytes = sailor_hip_surface_workspace_bytes(W, H, &band, 2);
    EXPECT(bytes == 64 + 1024 + (size_t)W * H * 8 + 2 * sizeof(SailorSurfaceDraw));
    // device pointers are never dereferenced on the host: aligned fakes
    alignas(16) static char fake[64];
    void* ws = fake;
    const auto* inst = reinterpret_cast<const SailorPerInstanceData*>(fake);
    const auto* mats = reinterpret_cast<const SailorMaterialData*>(fake);
    const auto* tex = reinterpret_cast<const SailorTextureDesc*>(fake);
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 1; d.flags = SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK;
    auto draw = [&](const SailorSurfaceDraw* dd, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt, uint32_t index,
                    const SailorBand* b, void* w, size_t n) { return sailor_hip_surface_draw_masked(&ctx, &frame, dd, i, m, nm, t, nt, index, W, H, b, w, n); };
    EXPECT(sailor_hip_surface_draw_masked(nullptr, &frame, &d, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_draw_masked(&ctx, nullptr, &d, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "frame or draw is NULL"));
    EXPECT(refused(ctx, draw(nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "frame or draw is NULL"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &bad, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, nullptr, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes), "workspace is NULL"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes), "not 16-byte aligned"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, ws, 0), "too small"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0, &band, ws, bytes - 2 * sizeof(SailorSurfaceDraw)), "too small"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 2, &band, ws, bytes), "drawIndex"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 1, 0xFFFFFFFFu, &band, ws, ~(size_t)0), "drawIndex"));
    EXPECT(refused(ctx, draw(&d, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 0, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, nullptr, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, inst, mats, 1, tex, 0, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes), "buffer is NULL"));
    for (uint32_t bit = 2; bit < 32; bit++) {
        SailorSurfaceDraw e = d;
        e.flags = d.flags | (1u << bit);
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "unknown flags"));
        e.flags = 1u << bit;
        EXPECT(refused(ctx, draw(&e, inst, nullptr, 0, nullptr, 0, 0, &band, ws, bytes), "unknown flags"));
    }
    {
        SailorSurfaceDraw e = d;
        e.dVertices = nullptr;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "buffer is NULL"));
        e = d; e.primBase = 0xFFFFFFFFu - 4u;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.primBase = 0xFFFFFFFFu;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.numTriangles = 0xFFFFFFFFu; e.numDrawn = 0xFFFFFFFFu;   // the product needs 64 bits
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
    }
    float* depth = reinterpret_cast<float*>(fake);
    EXPECT(sailor_hip_surface_store_depth(nullptr, ws, bytes, depth, W, H, &band) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, ws, bytes, depth, W, H, &bad), "band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, ws, bytes, depth, 0, H, &band), "band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, nullptr, bytes, depth, W, H, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, fake + 4, bytes, depth, W, H, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, ws, 64 + 1024 + (size_t)W * H * 8, depth, W, H, &band), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, ws, bytes, nullptr, W, H, &band), "depth attachment"));
    EXPECT(refused(ctx, sailor_hip_surface_store_depth(&ctx, ws, bytes, reinterpret_cast<float*>(fake + 2), W, H, &band), "depth attachment"));

    // ---- the harness's tag text ----
    std::vector<std::string> out;
    EXPECT(sailor_rt_parse_scene_tags("Opaque,Masked,,Masked", 4, out) && out.size() == 4 && out[0] == "Opaque" && out[1] == "Masked" && out[2].empty() && out[3] == "Masked");
    EXPECT(sailor_rt_parse_scene_tags(nullptr, 3, out) && out.size() == 3 && out[1].empty());
    EXPECT(sailor_rt_parse_scene_tags("", 1, out) && out.size() == 1 && out[0].empty());
    EXPECT(sailor_rt_parse_scene_tags("", 0, out) && out.empty());
    EXPECT(sailor_rt_parse_scene_tags(",", 2, out) && out.size() == 2);
    EXPECT(!sailor_rt_parse_scene_tags("a", 0, out) && out.empty());
    EXPECT(!sailor_rt_parse_scene_tags("a,b", 3, out) && out.empty());
    EXPECT(!sailor_rt_parse_scene_tags("a,b,c,d", 3, out) && out.empty());
    EXPECT(!sailor_rt_parse_scene_tags("a,b,c,", 3, out) && out.empty());
    EXPECT(!sailor_rt_parse_scene_tags("a b", 1, out) && !sailor_rt_parse_scene_tags("a;b", 1, out) && !sailor_rt_parse_scene_tags("\xff", 1, out));
    EXPECT(!sailor_rt_parse_scene_tags("a", -1, out));
    std::string longest(SAILOR_RT_TAG_MAX, 'x');
    EXPECT(sailor_rt_parse_scene_tags(longest.c_str(), 1, out) && out[0] == longest);
    EXPECT(!sailor_rt_parse_scene_tags((longest + "x").c_str(), 1, out));
    std::string many;
    for (int i = 0; i < 5000; i++) many += i ? ",T" : "T";
    EXPECT(sailor_rt_parse_scene_tags(many.c_str(), 5000, out) && out.size() == 5000 && !sailor_rt_parse_scene_tags(many.c_str(), 4999, out));
    const uint32_t flags[4] = { 0, 1, 2, 3 }, wrong[2] = { 1, 4 };
    EXPECT(sailor_rt_scene_flags_ok(flags, 4) && sailor_rt_scene_flags_ok(nullptr, 0) && !sailor_rt_scene_flags_ok(nullptr, 1) && !sailor_rt_scene_flags_ok(wrong, 2) &&
           !sailor_rt_scene_flags_ok(flags, -1));
    printf(failures ? "masked_host_check: %d FAILED\n" : "masked_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
