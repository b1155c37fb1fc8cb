// A stand-alone program over the host-side logic of the multisampled surface pass: every refusal of sailor_hip_surface_msaa_begin, _msaa_draw,
// _msaa_draw_gltf, _msaa_layer, _msaa_accumulate and _msaa_store_depth (argument checks, the sample counts, alignment, the store's size arithmetic, the
// layer range, k, the planes, the flag bits), sailor_hip_surface_msaa_bytes with its 0 cases, the sample table and the word it is packed into, built with
// the sanitizers on the host side, in the manner of scripts/bucket_host_check.cpp.  No GPU is needed or used: every call here is refused before anything
// is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/msaa_host_check.cpp -o /tmp/msaa_host_check -L. -lsailor_hip -Wl,-rpath,$PWD \
//       && /tmp/msaa_host_check
#include "../sailor_amd/csrc/surface_msaa.hip"
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
    const uint32_t S = 8;
    SailorBand band, bad, half;
    sailor_hip_band_whole_frame(W, H, &band);
    bad = band; bad.fbRowCount = H + 1;
    const size_t bytes = sailor_hip_surface_workspace_bytes(W, H, &band, 2);

    // ---- the sample table and its packed form ----
    for (uint32_t s : {1u, 2u, 4u, 8u}) {
        int32_t t[8][2];
        EXPECT(sailor_host_msaa_sample_positions(s, t) == SAILOR_HIP_OK);
        const unsigned long long p = msaa_pattern(s);
        long long sx = 0, sy = 0;
        for (uint32_t k = 0; k < s; k++) {
            EXPECT(t[k][0] % 16 == 0 && t[k][1] % 16 == 0 && t[k][0] >= 16 && t[k][0] <= 240 && t[k][1] >= 16 && t[k][1] <= 240);
            EXPECT((int)((p >> (8 * k)) & 15u) * 16 == t[k][0] && (int)((p >> (8 * k + 4)) & 15u) * 16 == t[k][1]);   // what surf_msaa_dx / _dy unpack, + 128
            sx += t[k][0]; sy += t[k][1];
        }
        EXPECT(sx == 128ll * s && sy == 128ll * s);   // the standard tables are centred on the pixel centre
        EXPECT(s == 8 || (p >> (8 * s)) == 0);
    }
    int32_t out[8][2];
    for (uint32_t s : {0u, 3u, 5u, 6u, 7u, 9u, 16u, 32u, 64u, 0xFFFFFFFFu}) EXPECT(sailor_host_msaa_sample_positions(s, out) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(sailor_host_msaa_sample_positions(8, nullptr) == SAILOR_HIP_ERR_INVALID_ARGUMENT);

    // ---- the size of the store ----
    const size_t store = sailor_hip_surface_msaa_bytes(W, &band, S);
    EXPECT(store == (size_t)S * W * H * 8);
    EXPECT(sailor_hip_surface_msaa_bytes(W, &band, 1) == (size_t)W * H * 8 && sailor_hip_surface_msaa_bytes(W, &band, 2) == (size_t)2 * W * H * 8 &&
           sailor_hip_surface_msaa_bytes(W, &band, 4) == (size_t)4 * W * H * 8);
    half = band; half.fbRowCount = 7;
    EXPECT(sailor_hip_surface_msaa_bytes(W, &half, S) == (size_t)S * W * 7 * 8);   // the band's rows, not the frame's
    half.fbRowCount = 2160;
    EXPECT(sailor_hip_surface_msaa_bytes(3840, &half, 8) == (size_t)530841600);     // 64 bytes a pixel: the 531 MB of DESIGN.md
    half.fbRowCount = 32768;
    EXPECT(sailor_hip_surface_msaa_bytes(32768, &half, 8) == (size_t)32768 * 32768 * 64);   // beyond 32 bits
    EXPECT(sailor_hip_surface_msaa_bytes(W, nullptr, S) == 0 && sailor_hip_surface_msaa_bytes(0, &band, S) == 0 && sailor_hip_surface_msaa_bytes(-3, &band, S) == 0);
    EXPECT(sailor_hip_surface_msaa_bytes(32769, &band, S) == 0);
    for (uint32_t s : {0u, 3u, 5u, 6u, 7u, 9u, 16u, 0xFFFFFFFFu}) EXPECT(sailor_hip_surface_msaa_bytes(W, &band, s) == 0);
    half = band; half.fbRowCount = 0;
    EXPECT(sailor_hip_surface_msaa_bytes(W, &half, S) == 0);
    half.fbRowCount = -1;
    EXPECT(sailor_hip_surface_msaa_bytes(W, &half, S) == 0);

    void* ws = fake;
    const auto* inst = reinterpret_cast<const SailorPerInstanceData*>(fake);
    const auto* mats = reinterpret_cast<const SailorMaterialData*>(fake);
    const auto* tex = reinterpret_cast<const SailorTextureDesc*>(fake);
    float* plane = reinterpret_cast<float*>(fake);
    float* plane4 = reinterpret_cast<float*>(fake + 4);   // 4-byte aligned, not 16
    float* odd2 = reinterpret_cast<float*>(fake + 2);
    void* st = fake;
    void* st8 = fake + 8;   // 8-byte aligned, not 16
    uint8_t* bytePlane = reinterpret_cast<uint8_t*>(fake + 1);   // a byte plane needs no alignment
    uint32_t* count = reinterpret_cast<uint32_t*>(fake);
    uint32_t* count2 = reinterpret_cast<uint32_t*>(fake + 2);
    SailorUboFrameData frame;
    memset(&frame, 0, sizeof frame);
    SailorSurfaceDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3N3T3B3UV2C4*>(fake); d.dIndices = reinterpret_cast<const uint32_t*>(fake);
    d.numTriangles = 2; d.numDrawn = 1;

    // ---- begin ----
    auto begin = [&](const SailorBand* b, void* w, size_t n, void* s, size_t sn, uint32_t samples, const float* z = nullptr, int32_t width = W) {
        return sailor_hip_surface_msaa_begin(&ctx, width, H, b, w, n, s, sn, samples, z);
    };
    EXPECT(sailor_hip_surface_msaa_begin(nullptr, W, H, &band, ws, bytes, st, store, S, nullptr) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, begin(&bad, ws, bytes, st, store, S), "msaa_begin: the band is not valid"));
    EXPECT(refused(ctx, begin(nullptr, ws, bytes, st, store, S), "band is not valid"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, st, store, S, nullptr, 0), "band is not valid"));
    EXPECT(refused(ctx, begin(&band, nullptr, bytes, st, store, S), "workspace is NULL"));
    EXPECT(refused(ctx, begin(&band, fake + 8, bytes, st, store, S), "not 16-byte aligned"));
    EXPECT(refused(ctx, begin(&band, ws, 64 + 1024 + (size_t)W * H * 8, st, store, S), "too small"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, nullptr, store, S), "sample store is NULL"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, st8, store, S), "not 16-byte aligned"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, st, store - 1, S), "smaller than sailor_hip_surface_msaa_bytes"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, st, sailor_hip_surface_msaa_bytes(W, &band, 4), S), "smaller than sailor_hip_surface_msaa_bytes"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, st, 0, 1), "smaller than sailor_hip_surface_msaa_bytes"));
    for (uint32_t s : {0u, 3u, 5u, 6u, 7u, 9u, 16u, 32u, 64u, 0xFFFFFFFFu}) EXPECT(refused(ctx, begin(&band, ws, bytes, st, ~(size_t)0, s), "samples is not 1, 2, 4 or 8"));
    EXPECT(refused(ctx, begin(&band, ws, bytes, st, store, S, odd2), "sample depth is not 4-byte aligned"));

    // ---- the layer read-out ----
    auto layer = [&](const SailorBand* b, void* w, size_t n, const void* s, size_t sn, uint32_t samples, uint32_t layers, uint32_t k, uint8_t* weight, uint8_t* un, uint32_t* c,
                     uint32_t* cl = nullptr) { return sailor_hip_surface_msaa_layer(&ctx, W, H, b, w, n, s, sn, samples, layers, k, weight, un, c, cl); };
    EXPECT(sailor_hip_surface_msaa_layer(nullptr, W, H, &band, ws, bytes, st, store, S, S, 0, bytePlane, bytePlane, count, nullptr) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, layer(&bad, ws, bytes, st, store, S, S, 0, bytePlane, bytePlane, count), "msaa_layer: the band is not valid"));
    EXPECT(refused(ctx, layer(&band, nullptr, bytes, st, store, S, S, 0, bytePlane, bytePlane, count), "workspace is NULL"));
    EXPECT(refused(ctx, layer(&band, ws, 100, st, store, S, S, 0, bytePlane, bytePlane, count), "too small"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, nullptr, store, S, S, 0, bytePlane, bytePlane, count), "sample store is NULL"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st8, store, S, S, 0, bytePlane, bytePlane, count), "not 16-byte aligned"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store - 8, S, S, 0, bytePlane, bytePlane, count), "smaller than sailor_hip_surface_msaa_bytes"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, ~(size_t)0, 3, 1, 0, bytePlane, bytePlane, count), "samples is not 1, 2, 4 or 8"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, 0, 0, bytePlane, bytePlane, count), "layers is outside 1 .. samples"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S + 1, 0, bytePlane, bytePlane, count), "layers is outside 1 .. samples"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, 2, 3, 0, bytePlane, bytePlane, count), "layers is outside 1 .. samples"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, 0xFFFFFFFFu, 0, bytePlane, bytePlane, count), "layers is outside 1 .. samples"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, 4, 4, bytePlane, bytePlane, count), "k is not below layers"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, S, bytePlane, bytePlane, count), "k is not below layers"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, 0xFFFFFFFFu, bytePlane, bytePlane, count), "k is not below layers"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, 1, nullptr, nullptr, count), "weight plane is NULL"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, 0, bytePlane, nullptr, count), "layer 0 needs the uncovered plane"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, 1, bytePlane, nullptr, nullptr), "counter"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, 1, bytePlane, nullptr, count2), "counter"));
    EXPECT(refused(ctx, layer(&band, ws, bytes, st, store, S, S, 1, bytePlane, nullptr, count, count2), "counter"));

    // ---- the accumulate ----
    auto acc = [&](const float* r, const float* e, const uint8_t* weight, const uint8_t* un, uint32_t samples, uint32_t k, float* t, const SailorBand* b = nullptr) {
        return sailor_hip_surface_msaa_accumulate(&ctx, r, e, weight, un, samples, k, t, W, H, b ? b : &band);
    };
    EXPECT(sailor_hip_surface_msaa_accumulate(nullptr, plane, nullptr, bytePlane, bytePlane, S, 0, plane, W, H, &band) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, bytePlane, S, 0, plane, &bad), "msaa_accumulate: the band is not valid"));
    EXPECT(refused(ctx, sailor_hip_surface_msaa_accumulate(&ctx, plane, nullptr, bytePlane, bytePlane, S, 0, plane, W, H, nullptr), "band is not valid"));
    for (uint32_t s : {0u, 3u, 16u}) EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, bytePlane, s, 0, plane), "samples is not 1, 2, 4 or 8"));
    EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, bytePlane, S, S, plane), "k is not below layers"));
    EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, bytePlane, 2, 2, plane), "k is not below layers"));
    EXPECT(refused(ctx, acc(plane, nullptr, nullptr, bytePlane, S, 0, plane), "weight plane is NULL"));
    EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, nullptr, S, 0, plane), "layer 0 needs the uncovered plane"));
    EXPECT(refused(ctx, acc(nullptr, nullptr, bytePlane, bytePlane, S, 0, plane), "colour plane"));
    EXPECT(refused(ctx, acc(plane4, nullptr, bytePlane, bytePlane, S, 0, plane), "colour plane"));
    EXPECT(refused(ctx, acc(plane, plane4, bytePlane, bytePlane, S, 0, plane), "colour plane"));
    EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, nullptr, S, 1, nullptr), "colour plane"));
    EXPECT(refused(ctx, acc(plane, nullptr, bytePlane, nullptr, S, 1, plane4), "colour plane"));

    // ---- the depth store ----
    auto depth = [&](const void* s, size_t sn, uint32_t samples, float* sd, float* z, const SailorBand* b = nullptr) {
        return sailor_hip_surface_msaa_store_depth(&ctx, s, sn, samples, sd, z, W, H, b ? b : &band);
    };
    EXPECT(sailor_hip_surface_msaa_store_depth(nullptr, st, store, S, plane, plane, W, H, &band) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, depth(st, store, S, plane, plane, &bad), "msaa_store_depth: the band is not valid"));
    EXPECT(refused(ctx, depth(nullptr, store, S, plane, plane), "sample store is NULL"));
    EXPECT(refused(ctx, depth(st8, store, S, plane, plane), "not 16-byte aligned"));
    EXPECT(refused(ctx, depth(st, store - 1, S, plane, plane), "smaller than sailor_hip_surface_msaa_bytes"));
    EXPECT(refused(ctx, depth(st, ~(size_t)0, 5, plane, plane), "samples is not 1, 2, 4 or 8"));
    EXPECT(refused(ctx, depth(st, store, S, nullptr, nullptr), "both outputs are NULL"));
    EXPECT(refused(ctx, depth(st, store, S, odd2, nullptr), "not 4-byte aligned"));
    EXPECT(refused(ctx, depth(st, store, S, nullptr, odd2), "not 4-byte aligned"));

    // ---- the two draws: everything the masked draws refuse, and the store ----
    for (int g = 0; g < 2; g++) {
        const auto entry = g ? sailor_hip_surface_msaa_draw_gltf : sailor_hip_surface_msaa_draw;
        const char* who = g ? "sailor_hip_surface_msaa_draw_gltf: " : "sailor_hip_surface_msaa_draw: ";
        SailorSurfaceDraw base = d;
        base.flags = SAILOR_SURFACE_ALPHA_CUTOUT | SAILOR_SURFACE_CULL_BACK | (g ? SAILOR_SURFACE_GLTF : 0u);
        auto draw = [&](const SailorSurfaceDraw* dd, const SailorPerInstanceData* i, const SailorMaterialData* m, uint32_t nm, const SailorTextureDesc* t, uint32_t nt,
                        uint32_t index, const SailorBand* b, void* w, size_t n, void* s = fake, size_t sn = ~(size_t)0, uint32_t samples = 8) {
            return entry(&ctx, &frame, dd, i, m, nm, t, nt, index, W, H, b, w, n, s, sn, samples);
        };
        EXPECT(entry(nullptr, &frame, &base, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes, st, store, S) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(refused(ctx, entry(&ctx, nullptr, &base, inst, mats, 1, tex, 1, 0, W, H, &band, ws, bytes, st, store, S), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(nullptr, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "frame or draw is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &bad, ws, bytes), who));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &bad, ws, bytes), "band is not valid"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, nullptr, bytes), "workspace is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, fake + 8, bytes), "not 16-byte aligned"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, 0), "too small"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 2, &band, ws, bytes), "drawIndex"));
        EXPECT(refused(ctx, draw(&base, inst, nullptr, 1, tex, 1, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 0, 0, &band, ws, bytes), "ALPHA_CUTOUT needs materials and textures"));
        EXPECT(refused(ctx, draw(&base, nullptr, mats, 1, tex, 1, 0, &band, ws, bytes), "buffer is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, nullptr), "sample store is NULL"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, st8), "not 16-byte aligned"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, st, store - 1), "smaller than sailor_hip_surface_msaa_bytes"));
        EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, st, sailor_hip_surface_msaa_bytes(W, &band, 2), 4), "smaller than sailor_hip_surface_msaa_bytes"));
        for (uint32_t s : {0u, 3u, 5u, 6u, 7u, 9u, 16u, 32u, 64u, 0xFFFFFFFFu})
            EXPECT(refused(ctx, draw(&base, inst, mats, 1, tex, 1, 0, &band, ws, bytes, st, ~(size_t)0, s), "samples is not 1, 2, 4 or 8"));
        for (uint32_t bit = 3; bit < 32; bit++) {   // the blend field of the Transparent queue among them
            SailorSurfaceDraw e = base;
            e.flags |= 1u << bit;
            EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "unknown flags"));
        }
        SailorSurfaceDraw e = base;
        e.primBase = 0xFFFFFFFFu - 4u;   // orderPlus1 would reach 2^32 - 1, the read-out's "no further order"
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), "reaches 2^32 - 1"));
        e = base; e.flags ^= SAILOR_SURFACE_GLTF;   // the glTF bit on the Standard entry, its absence on the glTF one
        EXPECT(refused(ctx, draw(&e, inst, mats, 1, tex, 1, 0, &band, ws, bytes), g ? "does not carry SAILOR_SURFACE_GLTF" : "unknown flags"));
    }
    printf(failures ? "msaa_host_check: %d FAILED\n" : "msaa_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
