// A stand-alone program over the host-side logic the indirect surface draw added: every refusal of sailor_hip_surface_draw_indirect (argument checks, the
// command's alignment, dInstanceIds, flag bits, the tables ALPHA_CUTOUT requires, the 2^32 - 1 arithmetic on the CAPACITY) and the command's layout, built with
// the sanitizers on the host side.  No GPU is needed or used: every call here is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/indirect_host_check.cpp -o /tmp/indirect_host_check -L. -lsailor_hip -Wl,-rpath,$PWD && /tmp/indirect_host_check
#include "../sailor_amd/csrc/surface_indirect.hip"
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static bool refused(SailorHipContext& ctx, int status, const char* text)
{
    const bool ok = status == SAILOR_HIP_ERR_INVALID_ARGUMENT && ctx.launchCount == 0 && ctx.lastError.find("sailor_hip_surface_draw_indirect") != std::string::npos &&
                    ctx.lastError.find(text) != std::string::npos;
    if (!ok) printf("  status %d, launches %llu, last_error '%s', wanted '%s'\n", status, (unsigned long long)ctx.launchCount, ctx.lastError.c_str(), text);
    ctx.lastError.clear();
    return ok;
}

int main()
{
    // RHI/Types.h DrawIndexedIndirectData == VkDrawIndexedIndirectCommand: the kernel reads words 1 and 4
    static_assert(sizeof(SailorDrawIndexedIndirectData) == 20 && offsetof(SailorDrawIndexedIndirectData, instanceCount) == 4 &&
                  offsetof(SailorDrawIndexedIndirectData, firstInstance) == 16, "the command's layout");
    static_assert(sizeof(SailorSurfaceDraw) == 48 && offsetof(SailorSurfaceDraw, numDrawn) == 28 && offsetof(SailorSurfaceDraw, firstInstance) == 40, "the descriptor's layout");
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
    const auto* cmd = reinterpret_cast<const SailorDrawIndexedIndirectData*>(fake + 20);   // the second command of a buffer: 4-byte aligned, not 8
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 6; d.flags = SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK;
    auto draw = [&](const SailorSurfaceDraw* dd, const SailorDrawIndexedIndirectData* c, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm,
                    const SailorTextureDesc* t, uint32_t nt, uint32_t index, const SailorBand* b, void* w, size_t n) {
        return sailor_hip_surface_draw_indirect(&ctx, &frame, dd, c, i, 7, m, nm, t, nt, index, W, H, b, w, n);
    };
    EXPECT(sailor_hip_surface_draw_indirect(nullptr, &frame, &d, cmd, inst, 7, mats, 1, tex, 1, 0, W, H, &band, ws, bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_draw_indirect(&ctx, nullptr, &d, cmd, inst, 7, mats, 1, tex, 1, 0, W, H, &band, ws, bytes), "frame or draw is NULL"));
    EXPECT(refused(ctx, draw(nullptr, cmd, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "frame or draw is NULL"));
    EXPECT(refused(ctx, draw(&d, nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "command is NULL or not 4-byte aligned"));
    for (int off = 1; off < 4; off++)
        EXPECT(refused(ctx, draw(&d, reinterpret_cast<const SailorDrawIndexedIndirectData*>(fake + off), inst, mats, 1, tex, 1, 0, &band, ws, bytes), "not 4-byte aligned"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 1, 0, &bad, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 1, 0, nullptr, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes), "workspace is NULL"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes), "not 16-byte aligned"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 1, 0, &band, ws, 0), "too small"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 1, 2, &band, ws, bytes), "drawIndex"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 0, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, nullptr, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, cmd, inst, mats, 1, tex, 0, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
    EXPECT(refused(ctx, draw(&d, cmd, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes), "buffer is NULL"));
    for (uint32_t bit = 3; bit < 32; bit++) {
        SailorSurfaceDraw e = d;
        e.flags = d.flags | (1u << bit);
        EXPECT(refused(ctx, draw(&e, cmd, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "unknown flags"));
    }
    {
        SailorSurfaceDraw e = d;
        e.dInstanceIds = reinterpret_cast<const uint32_t*>(fake);
        EXPECT(refused(ctx, draw(&e, cmd, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "dInstanceIds must be NULL"));
        e = d; e.flags |= SAILOR_SURFACE_GLTF;   // the glTF kernel's cutout needs the tables as well
        EXPECT(refused(ctx, draw(&e, cmd, inst, nullptr, 0, nullptr, 0, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        // the 2^32 - 1 refusal is the CAPACITY's: 6 instances x 2 triangles x 2 parts = 24 orders
        e = d; e.primBase = 0xFFFFFFFFu - 24u;
        EXPECT(refused(ctx, draw(&e, cmd, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.numTriangles = 0xFFFFFFFFu; e.numDrawn = 0xFFFFFFFFu;   // the product needs 64 bits
        EXPECT(refused(ctx, draw(&e, cmd, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.numDrawn = 0x40000000u;                                  // more lanes than a grid of 2^31 - 1 holds
        EXPECT(refused(ctx, draw(&e, cmd, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
    }
    printf(failures ? "indirect_host_check: %d FAILED\n" : "indirect_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
