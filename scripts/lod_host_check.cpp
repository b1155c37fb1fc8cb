// A stand-alone program over the host-side logic the mip-mapped textures added: every refusal of sailor_hip_texture_generate_mips,
// sailor_hip_surface_resolve_lod, sailor_hip_surface_draw_lod and sailor_hip_surface_draw_indirect_lod (argument checks, flag bits, the tables ALPHA_CUTOUT
// requires, alignment, the workspace's size arithmetic), the descriptor's layout, the level count, the chain offsets and the encode table, built with the
// sanitizers on the host side.  No GPU is needed or used: every call here is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/lod_host_check.cpp -o /tmp/lod_host_check -L. -lsailor_hip -Wl,-rpath,$PWD && /tmp/lod_host_check
#include "../sailor_amd/csrc/surface_lod.hip"
#include "../sailor_amd/csrc/texture_mips.hip"
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
    static_assert(sizeof(SailorTextureDesc) == 24 && offsetof(SailorTextureDesc, flags) == 16 && offsetof(SailorTextureDesc, levels) == 20, "the field took the padding's place");
    // ---- the level count and the chain offsets ----
    const int32_t extents[][2] = { { 8, 8 }, { 5, 3 }, { 16, 4 }, { 17, 9 }, { 1, 7 }, { 1, 1 }, { 64, 64 }, { 32768, 32768 }, { 32768, 1 }, { 3, 32767 }, { 1000, 513 } };
    for (const auto& e : extents) {
        const int32_t w = e[0], h = e[1], m = w > h ? w : h;
        uint32_t full = 0;
        while ((m >> full) > 0) full++;
        EXPECT(sailor_hip_texture_mip_levels(w, h) == full && (uint32_t)surf_full_levels(w, h) == full);
        EXPECT(surf_level_count(w, h, 0) == 1 && surf_level_count(w, h, 1) == 1 && surf_level_count(w, h, full) == (int)full && surf_level_count(w, h, 99) == (int)full &&
               surf_level_count(w, h, 0xFFFFFFFFu) == (int)full);
        size_t sum = 0;
        for (uint32_t l = 0; l <= full; l++) {
            EXPECT(surf_level_offset(w, h, (int)l) == sum && sailor_hip_mip_chain_texels(w, h, (int32_t)l) == sum);
            sum += (size_t)surf_level_extent(w, (int)l) * (size_t)surf_level_extent(h, (int)l);
        }
        EXPECT(surf_level_extent(m, (int)full - 1) == 1 && (full < 2 || surf_level_extent(m, (int)full - 2) > 1)); // the last level is 1 x 1, the one before it is not
    }
    EXPECT(sailor_hip_texture_mip_levels(0, 4) == 0 && sailor_hip_texture_mip_levels(4, 0) == 0 && sailor_hip_texture_mip_levels(-1, 4) == 0 &&
           sailor_hip_texture_mip_levels(32769, 1) == 0 && sailor_hip_texture_mip_levels(1, 32769) == 0);
    EXPECT(sailor_hip_mip_chain_texels(32768, 32768, 16) < (1ull << 32)); // a whole chain's texel offsets fit 32 bits
    // ---- the encode table: strictly rising, every byte's decode strictly between its two boundaries ----
    float dec[256], enc[255];
    EXPECT(sailor_host_srgb_encode_table(nullptr) == SAILOR_HIP_ERR_INVALID_ARGUMENT && sailor_host_srgb_encode_table(enc) == SAILOR_HIP_OK && sailor_host_srgb_table(dec) == SAILOR_HIP_OK);
    for (int k = 0; k < 255; k++) EXPECT(dec[k] < enc[k] && enc[k] < dec[k + 1] && (k == 0 || enc[k - 1] < enc[k]));

    SailorHipContext ctx;
    alignas(16) static char fake[64]; // device pointers are never dereferenced on the host: aligned fakes
    uint32_t* texels = reinterpret_cast<uint32_t*>(fake);
    // ---- sailor_hip_texture_generate_mips ----
    EXPECT(sailor_hip_texture_generate_mips(nullptr, texels, 8, 8, 4, 0) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, nullptr, 8, 8, 4, 0), "texels are NULL"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, reinterpret_cast<uint32_t*>(fake + 2), 8, 8, 4, 0), "not 4-byte aligned"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, reinterpret_cast<uint32_t*>(fake + 1), 8, 8, 4, 0), "not 4-byte aligned"));
    const int32_t badExtents[][2] = { { 0, 8 }, { 8, 0 }, { -1, 8 }, { 8, -8 }, { 32769, 8 }, { 8, 32769 }, { INT32_MIN, 8 }, { INT32_MAX, INT32_MAX } };
    for (const auto& e : badExtents) EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, e[0], e[1], 1, 0), "outside 1 .. 32768"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, 8, 8, 0, 0), "levels is outside"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, 8, 8, 5, 0), "levels is outside"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, 17, 9, 6, SAILOR_TEXTURE_SRGB), "levels is outside"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, 1, 1, 2, 0), "levels is outside"));
    EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, 8, 8, 0xFFFFFFFFu, 0), "levels is outside"));
    for (uint32_t bit = 1; bit < 32; bit++) EXPECT(refused(ctx, sailor_hip_texture_generate_mips(&ctx, texels, 8, 8, 4, SAILOR_TEXTURE_SRGB | (1u << bit)), "unknown flags"));
    // one level is nothing to do, with or without the flag: accepted, nothing launched
    EXPECT(sailor_hip_texture_generate_mips(&ctx, texels, 8, 8, 1, SAILOR_TEXTURE_SRGB) == SAILOR_HIP_OK && sailor_hip_texture_generate_mips(&ctx, texels, 1, 1, 1, 0) == SAILOR_HIP_OK &&
           ctx.launchCount == 0);

    // ---- the draws and the resolve ----
    const int32_t W = 40, H = 24;
    SailorBand band, bad;
    sailor_hip_band_whole_frame(W, H, &band);
    bad = band; bad.fbRowCount = H + 1;
    const size_t bytes = sailor_hip_surface_workspace_bytes(W, H, &band, 2);
    void* ws = fake;
    const auto* inst = reinterpret_cast<const SailorPerInstanceData*>(fake);
    const auto* mats = reinterpret_cast<const SailorMaterialData*>(fake);
    const auto* tex = reinterpret_cast<const SailorTextureDesc*>(fake);
    const auto* command = reinterpret_cast<const SailorDrawIndexedIndirectData*>(fake);
    float* plane = reinterpret_cast<float*>(fake);
    float* odd4 = reinterpret_cast<float*>(fake + 4);
    float* odd2 = reinterpret_cast<float*>(fake + 2);
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 1; d.flags = SAILOR_SURFACE_GLTF | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK;
    for (int indirect = 0; indirect < 2; indirect++) {
        const char* who = indirect ? "sailor_hip_surface_draw_indirect_lod: " : "sailor_hip_surface_draw_lod: ";
        auto draw = [&](const SailorUboFrameData* f, const SailorSurfaceDraw* dd, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t,
                        uint32_t nt, uint32_t index, const SailorBand* b, void* w, size_t n) {
            return indirect ? sailor_hip_surface_draw_indirect_lod(&ctx, f, dd, command, i, 8, m, nm, t, nt, index, W, H, b, w, n)
                            : sailor_hip_surface_draw_lod(&ctx, f, dd, i, m, nm, t, nt, index, W, H, b, w, n);
        };
        EXPECT((indirect ? sailor_hip_surface_draw_indirect_lod(nullptr, &frame, &d, command, inst, 8, mats, 1, tex, 1, 0, W, H, &band, ws, bytes)
                         : sailor_hip_surface_draw_lod(nullptr, &frame, &d, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes)) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(refused(ctx, draw(nullptr, &d, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(&frame, nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 1, 0, &bad, ws, bytes), "band is not valid"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 1, 0, nullptr, ws, bytes), "band is not valid"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes), "workspace is NULL"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes), "not 16-byte aligned"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 1, 0, &band, ws, 0), "too small"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 1, 2, &band, ws, bytes), "drawIndex"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 0, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, nullptr, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&frame, &d, inst, mats, 1, tex, 0, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&frame, &d, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes), "buffer is NULL"));
        for (uint32_t bit = 3; bit < 32; bit++) {
            SailorSurfaceDraw e = d;
            e.flags = d.flags | (1u << bit);
            EXPECT(refused(ctx, draw(&frame, &e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "unknown flags"));
        }
        SailorSurfaceDraw e = d;
        e.primBase = 0xFFFFFFFFu - 4u;
        EXPECT(refused(ctx, draw(&frame, &e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.numTriangles = 0xFFFFFFFFu; e.numDrawn = 0xFFFFFFFFu;   // the product needs 64 bits
        EXPECT(refused(ctx, draw(&frame, &e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.dVertices = nullptr;
        ctx.lastError.clear();
        EXPECT(draw(&frame, &e, inst, mats, 1, tex, 1, 0, &band, ws, bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT && ctx.lastError.rfind(who, 0) == 0); // the entry's own name in front
    }
    // the indirect entry's own checks
    EXPECT(refused(ctx, sailor_hip_surface_draw_indirect_lod(&ctx, &frame, &d, nullptr, inst, 8, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "command is NULL or not 4-byte aligned"));
    EXPECT(refused(ctx, sailor_hip_surface_draw_indirect_lod(&ctx, &frame, &d, reinterpret_cast<const SailorDrawIndexedIndirectData*>(fake + 2), inst, 8, mats, 1, tex, 1, 0, W, H, &band,
                                                             ws, bytes), "command is NULL or not 4-byte aligned"));
    {
        SailorSurfaceDraw e = d;
        e.dInstanceIds = reinterpret_cast<const uint32_t*>(fake);
        EXPECT(refused(ctx, sailor_hip_surface_draw_indirect_lod(&ctx, &frame, &e, command, inst, 8, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "dInstanceIds must be NULL"));
    }
    auto resolve = [&](const SailorUboFrameData* f, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt, const SailorBand* b,
                       const void* w, size_t n, float* surface, size_t stride, float* depth, const float* aoIn, float* aoOut, float* emissive) {
        return sailor_hip_surface_resolve_lod(&ctx, f, i, m, nm, t, nt, W, H, b, w, n, surface, stride, depth, nullptr, aoIn, aoOut, emissive);
    };
    const size_t px = (size_t)W * H;
    EXPECT(sailor_hip_surface_resolve_lod(nullptr, &frame, inst, mats, 1, tex, 1, W, H, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, nullptr, plane) ==
           SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, resolve(nullptr, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(&frame, nullptr, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(&frame, inst, nullptr, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 0, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, nullptr, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 0, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "missing"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &bad, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane), "band is not valid"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, nullptr, bytes, plane, px, nullptr, nullptr, nullptr, plane), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, 64 + 1024 + px * 8, plane, px, nullptr, nullptr, nullptr, plane), "workspace is NULL, misaligned or too small"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, nullptr, px, nullptr, nullptr, nullptr, plane), "surface is NULL"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, odd4, px, nullptr, nullptr, nullptr, plane), "surface is NULL or not 16-byte aligned"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px - 1, nullptr, nullptr, nullptr, plane), "planeStride"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, odd2, nullptr, nullptr, plane), "depth output is misaligned"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, odd2, nullptr, plane), "occlusion plane is misaligned"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, odd2, plane), "occlusion plane is misaligned"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, nullptr), "emissive plane is NULL"));
    EXPECT(refused(ctx, resolve(&frame, inst, mats, 1, tex, 1, &band, ws, bytes, plane, px, nullptr, nullptr, nullptr, odd4), "emissive plane is NULL or not 16-byte aligned"));
    ctx.lastError.clear();
    EXPECT(resolve(&frame, inst, mats, 1, tex, 1, &bad, ws, bytes, plane, px, nullptr, nullptr, nullptr, plane) == SAILOR_HIP_ERR_INVALID_ARGUMENT &&
           ctx.lastError.rfind("sailor_hip_surface_resolve_lod: ", 0) == 0);
    printf(failures ? "lod_host_check: %d FAILED\n" : "lod_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
