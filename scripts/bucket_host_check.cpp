// A stand-alone program over the host-side logic of the Transparent queue's bucket route: every refusal of sailor_hip_surface_bucket_begin, _bucket_draw,
// _bucket_draw_gltf and _bucket_layer (argument checks, the flag bits and the blend field, MULTIPLY's unsupported status, alignment, the store's size
// arithmetic, the layer range, k) and sailor_hip_surface_bucket_bytes with its 0 cases, built with the sanitizers on the host side, in the manner of
// scripts/transparent_host_check.cpp.  No GPU is needed or used: every call here is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/bucket_host_check.cpp -o /tmp/bucket_host_check -L. -lsailor_hip -Wl,-rpath,$PWD \
//       && /tmp/bucket_host_check
#include "../sailor_amd/csrc/surface_buckets.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int failures = 0;
alignas(16) static char fake[64];   // device pointers are never dereferenced on the host: aligned fakes
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
    SailorHipContext ctx;
    const int32_t W = 50, H = 35;
    const uint32_t K = 4;
    SailorBand band, bad, half;
    sailor_hip_band_whole_frame(W, H, &band);
    bad = band; bad.fbRowCount = H + 1;
    const size_t bytes = sailor_hip_surface_workspace_bytes(W, H, &band, 2);

    // ---- the size of the store ----
    const size_t store = sailor_hip_surface_bucket_bytes(W, &band, K);
    EXPECT(store == (size_t)(K + 1) * W * H * 8);
    EXPECT(sailor_hip_surface_bucket_bytes(W, &band, 1) == (size_t)2 * W * H * 8 && sailor_hip_surface_bucket_bytes(W, &band, 64) == (size_t)65 * W * H * 8);
    half = band; half.fbRowCount = 7;
    EXPECT(sailor_hip_surface_bucket_bytes(W, &half, K) == (size_t)(K + 1) * W * 7 * 8);   // the band's rows, not the frame's
    half.fbRowCount = 2160;
    EXPECT(sailor_hip_surface_bucket_bytes(3840, &half, 64) == (size_t)65 * 3840 * 2160 * 8);   // 4.3 GB: beyond 32 bits
    EXPECT(sailor_hip_surface_bucket_bytes(W, nullptr, K) == 0 && sailor_hip_surface_bucket_bytes(0, &band, K) == 0 && sailor_hip_surface_bucket_bytes(-3, &band, K) == 0);
    EXPECT(sailor_hip_surface_bucket_bytes(32769, &band, K) == 0 && sailor_hip_surface_bucket_bytes(W, &band, 0) == 0 && sailor_hip_surface_bucket_bytes(W, &band, 65) == 0);
    half = band; half.fbRowCount = 0;
    EXPECT(sailor_hip_surface_bucket_bytes(W, &half, K) == 0);
    half.fbRowCount = -1;
    EXPECT(sailor_hip_surface_bucket_bytes(W, &half, K) == 0);

    void* ws = fake;
    const auto* inst = reinterpret_cast<const SailorPerInstanceData*>(fake);
    const auto* mats = reinterpret_cast<const SailorMaterialData*>(fake);
    const auto* tex = reinterpret_cast<const SailorTextureDesc*>(fake);
    float* plane = reinterpret_cast<float*>(fake);
    float* odd2 = reinterpret_cast<float*>(fake + 2);
    void* buckets = fake;
    void* buckets4 = fake + 4;   // 4-byte aligned, not 8
    uint32_t* count = reinterpret_cast<uint32_t*>(fake);
    uint32_t* count2 = reinterpret_cast<uint32_t*>(fake + 2);
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 1;
    const uint32_t ALPHA = SAILOR_SURFACE_BLEND_ALPHA << SAILOR_SURFACE_BLEND_SHIFT, MULTIPLY = SAILOR_SURFACE_BLEND_MULTIPLY << SAILOR_SURFACE_BLEND_SHIFT;

    // ---- begin ----
    EXPECT(sailor_hip_surface_bucket_begin(nullptr, W, H, &band, ws, bytes, buckets, store, K) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &bad, ws, bytes, buckets, store, K), "bucket_begin: the band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, nullptr, ws, bytes, buckets, store, K), "band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, 0, H, &band, ws, bytes, buckets, store, K), "band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, nullptr, bytes, buckets, store, K), "workspace is NULL"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, fake + 8, bytes, buckets, store, K), "not 16-byte aligned"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, 64 + 1024 + (size_t)W * H * 8, buckets, store, K), "too small"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, nullptr, store, K), "bucket store is NULL"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets4, store, K), "not 8-byte aligned"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets, store - 1, K), "smaller than sailor_hip_surface_bucket_bytes"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets, store, K + 1), "smaller than sailor_hip_surface_bucket_bytes"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets, 0, K), "smaller than sailor_hip_surface_bucket_bytes"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets, ~(size_t)0, 0), "layers is outside 1 .. 64"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets, ~(size_t)0, 65), "layers is outside 1 .. 64"));
    EXPECT(refused(ctx, sailor_hip_surface_bucket_begin(&ctx, W, H, &band, ws, bytes, buckets, ~(size_t)0, 0xFFFFFFFFu), "layers is outside 1 .. 64"));

    // ---- the layer read-out ----
    auto layer = [&](const SailorBand* b, void* w, size_t n, const void* s, size_t sn, uint32_t layers, uint32_t k, uint32_t* c) {
        return sailor_hip_surface_bucket_layer(&ctx, W, H, b, w, n, s, sn, layers, k, c);
    };
    EXPECT(sailor_hip_surface_bucket_layer(nullptr, W, H, &band, ws, bytes, buckets, store, K, 0, count) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, layer(&bad, ws, bytes, buckets, store, K, 0, count), "bucket_layer: the band is not valid"));
    EXPECT(refused(ctx, layer(&band, nullptr, bytes, buckets, store, K, 0, count), "workspace is NULL"));
    EXPECT(refused(ctx, layer(&band, ws, 100, buckets, store, K, 0, count), "too small"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, nullptr, store, K, 0, count), "bucket store is NULL"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets4, store, K, 0, count), "not 8-byte aligned"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, store - 8, K, 0, count), "smaller than sailor_hip_surface_bucket_bytes"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, ~(size_t)0, 0, 0, count), "layers is outside 1 .. 64"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, ~(size_t)0, 65, 0, count), "layers is outside 1 .. 64"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, store, K, K + 1, count), "k is beyond layers"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, store, K, 0xFFFFFFFFu, count), "k is beyond layers"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, store, K, 0, nullptr), "counter"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, buckets, store, K, K, count2), "counter"));

    // ---- the two draws: everything the peel draws refuse, and the store ----
    for (int g = 0; g < 2; g++) {
        const auto entry = g ? sailor_hip_surface_bucket_draw_gltf : sailor_hip_surface_bucket_draw;
        const char* who = g ? "sailor_hip_surface_bucket_draw_gltf: " : "sailor_hip_surface_bucket_draw: ";
        SailorSurfaceDraw base = d;
        base.flags = ALPHA | SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK | (g ? SAILOR_SURFACE_GLTF : 0u);
        auto draw = [&](const SailorSurfaceDraw* dd, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt,
                        uint32_t index, const SailorBand* b, void* w, size_t n, const float* depth, void* s = fake, size_t sn = ~(size_t)0, uint32_t layers = 4) {
            return entry(&ctx, &frame, dd, i, m, nm, t, nt, index, W, H, b, w, n, depth, s, sn, layers);
        };
        EXPECT(entry(nullptr, &frame, &base, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes, plane, buckets, store, K) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(refused(ctx, entry(&ctx, nullptr, &base, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes, plane, buckets, store, K), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &bad, ws, bytes, plane), who));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &bad, ws, bytes, plane), "band is not valid"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes, plane), "workspace is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes, plane), "not 16-byte aligned"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, 0, plane), "too small"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 2, &band, ws, bytes, plane), "drawIndex"));
        EXPECT(refused(ctx, draw(&base, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes, plane), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 0, 0, &band, ws, bytes, plane), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&base, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes, plane), "buffer is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, nullptr), "depth attachment"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, odd2), "depth attachment"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, nullptr), "bucket store is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, buckets4), "not 8-byte aligned"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, buckets, store - 1), "smaller than sailor_hip_surface_bucket_bytes"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, buckets, store, K + 1), "smaller than sailor_hip_surface_bucket_bytes"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, buckets, store, 0), "layers is outside 1 .. 64"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane, buckets, ~(size_t)0, 65), "layers is outside 1 .. 64"));
        for (uint32_t bit = 5; bit < 32; bit++) {
            SailorSurfaceDraw e = base;
            e.flags |= 1u << bit;
            EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane), "unknown flags"));
        }
        SailorSurfaceDraw e = base;
        e.flags = (base.flags & ~ALPHA) | MULTIPLY;
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane), "Multiply", SAILOR_HIP_ERR_UNSUPPORTED));
        e = base; e.primBase = 0xFFFFFFFFu - 4u;   // orderPlus1 would reach 2^32 - 1: EMPTY's high word stays out of reach
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane), "reaches 2^32 - 1"));
        e = base; e.flags ^= SAILOR_SURFACE_GLTF;   // the glTF bit on the Standard entry, its absence on the glTF one
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes, plane), g ? "does not carry SAILOR_SURFACE_GLTF" : "unknown flags"));
    }
    printf(failures ? "bucket_host_check: %d FAILED\n" : "bucket_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
