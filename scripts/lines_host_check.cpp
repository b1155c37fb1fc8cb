// A stand-alone program over the host-side logic the DebugDraw pass added: every refusal of sailor_hip_debug_lines_draw / _resolve / _prims (argument checks, the
// order range, the workspace's size arithmetic) and the DebugContext mirror (sailor_amd/runtime/Runtime/RHI/DebugContext.cpp) -- the shapes' segment counts and
// order, the lifetimes with RemoveAtSwap, the index growth --, built with the sanitizers on the host side.  No GPU is needed or used: every call of the library is
// refused before anything is launched, and the DebugContext is driven without a driver (ExpireLines / GrowIndices are the driver-free halves of Tick).
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/lines_host_check.cpp -o /tmp/lines_host_check -L. -lsailor_hip -Wl,-rpath,$PWD && /tmp/lines_host_check
#include "../sailor_amd/csrc/debug_lines.hip"
#include "../sailor_amd/runtime/Runtime/RHI/DebugContext.cpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

// the two accessors DebugContext::Tick would use (defined by the HIP driver in the library proper): there is no driver here, and Tick is not called
Sailor::RHI::IGraphicsDriver* Sailor::RHI::Renderer::s_driver = nullptr;
Sailor::RHI::IGraphicsDriverCommands* Sailor::RHI::Renderer::s_commands = nullptr;
Sailor::RHI::RHIBuffer::~RHIBuffer() {}

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
    const size_t bytes = sailor_hip_surface_workspace_bytes(W, H, &band, 1);
    alignas(16) static char fake[64]; // device pointers are never dereferenced on the host: aligned fakes
    void* ws = fake;
    float vp[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    SailorDebugLinesDraw d;
    memset(&d, 0, sizeof d);
    d.dVertices = reinterpret_cast<const SailorVertexP3C4*>(fake); d.numSegments = 3;
    EXPECT(sizeof(SailorDebugLinesDraw) == 24 && sizeof(SailorVertexP3C4) == 28);
    auto draw = [&](const float* m, const SailorDebugLinesDraw* dd, int32_t w, const SailorBand* b, void* p, size_t n) {
        return sailor_hip_debug_lines_draw(&ctx, m, dd, w, H, b, p, n);
    };
    float* depth = reinterpret_cast<float*>(fake);
    auto resolve = [&](const SailorDebugLinesDraw* dd, const SailorBand* b, const void* p, size_t n, float* t, float* z) {
        return sailor_hip_debug_lines_resolve(&ctx, vp, dd, W, H, b, p, n, t, z);
    };
    EXPECT(sailor_hip_debug_lines_draw(nullptr, vp, &d, W, H, &band, ws, bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(sailor_hip_debug_lines_resolve(nullptr, vp, &d, W, H, &band, ws, bytes, depth, depth) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(refused(ctx, draw(nullptr, &d, W, &band, ws, bytes), "the matrix or the draw is NULL"));
    EXPECT(refused(ctx, draw(vp, nullptr, W, &band, ws, bytes), "the matrix or the draw is NULL"));
    EXPECT(refused(ctx, draw(vp, &d, W, &bad, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(vp, &d, W, nullptr, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(vp, &d, 0, &band, ws, bytes), "band is not valid"));
    EXPECT(refused(ctx, draw(vp, &d, W, &band, nullptr, bytes), "workspace is NULL"));
    EXPECT(refused(ctx, draw(vp, &d, W, &band, fake + 8, bytes), "not 16-byte aligned"));
    EXPECT(refused(ctx, draw(vp, &d, W, &band, ws, 0), "too small"));
    EXPECT(refused(ctx, draw(vp, &d, W, &band, ws, bytes - 1), "too small"));
    {
        SailorDebugLinesDraw e = d;
        e.dVertices = nullptr;
        EXPECT(refused(ctx, draw(vp, &e, W, &band, ws, bytes), "vertex buffer"));
        e = d; e.dVertices = reinterpret_cast<const SailorVertexP3C4*>(fake + 2);
        EXPECT(refused(ctx, draw(vp, &e, W, &band, ws, bytes), "vertex buffer"));
        e = d; e.dIndices = reinterpret_cast<const uint32_t*>(fake + 1);
        EXPECT(refused(ctx, draw(vp, &e, W, &band, ws, bytes), "index buffer"));
        e = d; e.primBase = 0xFFFFFFFFu - 3u; // + 3 segments = 2^32 - 1
        EXPECT(refused(ctx, draw(vp, &e, W, &band, ws, bytes), "reaches 2^32 - 1"));
        EXPECT(refused(ctx, resolve(&e, &band, ws, bytes, depth, depth), "reaches 2^32 - 1"));
        e = d; e.primBase = 0xFFFFFFFFu; e.numSegments = 0xFFFFFFFFu; // the sum needs 64 bits
        EXPECT(refused(ctx, draw(vp, &e, W, &band, ws, bytes), "reaches 2^32 - 1"));
        e = d; e.numSegments = 0; e.dVertices = nullptr; // an empty draw is accepted and records nothing
        EXPECT(draw(vp, &e, W, &band, ws, bytes) == SAILOR_HIP_OK && ctx.launchCount == 0);
        EXPECT(resolve(&e, &band, ws, bytes, depth, depth) == SAILOR_HIP_OK && ctx.launchCount == 0);
    }
    EXPECT(refused(ctx, resolve(&d, &bad, ws, bytes, depth, depth), "band is not valid"));
    EXPECT(refused(ctx, resolve(&d, &band, nullptr, bytes, depth, depth), "workspace is NULL"));
    EXPECT(refused(ctx, resolve(&d, &band, ws, 64, depth, depth), "too small"));
    EXPECT(refused(ctx, resolve(&d, &band, ws, bytes, nullptr, depth), "the target is NULL"));
    EXPECT(refused(ctx, resolve(&d, &band, ws, bytes, reinterpret_cast<float*>(fake + 4), depth), "not 16-byte aligned"));
    EXPECT(refused(ctx, resolve(&d, &band, ws, bytes, depth, nullptr), "depth attachment"));
    EXPECT(refused(ctx, resolve(&d, &band, ws, bytes, depth, reinterpret_cast<float*>(fake + 2)), "depth attachment"));
    uint64_t prims = 1;
    EXPECT(sailor_hip_debug_lines_prims(7, nullptr) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
    EXPECT(sailor_hip_debug_lines_prims(0xFFFFFFFFu, &prims) == SAILOR_HIP_OK && prims == 0xFFFFFFFFull);

    // ---- the DebugContext mirror ----
    using Sailor::RHI::DebugContext;
    DebugContext dc;
    const float lo[3] = { -1, 2, 3 }, hi[3] = { 4, 5, 7 }, white[4] = { 1, 1, 1, 1 }, red[4] = { 1, 0, 0, 1 };
    dc.DrawAABB(lo, hi, red, 0.25f);
    EXPECT(dc.GetLineVertices().size() == 24 && dc.GetLifetimes().size() == 12 && dc.GetLineVerticesOffset() == 0);
    EXPECT(dc.GetLineVertices()[1].position[0] == 4 && dc.GetLineVertices()[1].position[1] == 2 && dc.GetLineVertices()[23].position[0] == -1);
    dc.DrawSphere(lo, 2.0f, white, 1.0f);
    EXPECT(dc.GetLifetimes().size() == 12 + 8 * (1 + 7 * 3));
    float corners[24];
    for (int k = 0; k < 24; k++) corners[k] = (float)k;
    dc.DrawFrustum(corners, red, 2.0f);
    const float eye[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    dc.DrawOrigin(lo, eye, 3.0f, 0.0f);
    dc.DrawArrow(lo, hi, white, 0.05f);
    const size_t lines = 12 + 176 + 12 + 3 + 4;
    EXPECT(dc.GetLifetimes().size() == lines && dc.GetLineVertices().size() == 2 * lines);
    EXPECT(dc.GetLineVertices()[2 * (12 + 176 + 12) + 1].position[0] == 2.0f); // the x axis: position + (3, 0, 0)
    EXPECT(dc.GrowIndices() && dc.GetCachedIndices().size() == 2 * lines && dc.GetCachedIndices()[2 * lines - 1] == 2 * lines - 1 && !dc.GrowIndices());
    EXPECT(dc.GetNumRenderedVertices() == 0); // only Tick sets it
    dc.ExpireLines(0.1f); // the origin's axes (0) and the arrow (0.05) leave; they were the last lines, so the buffer changed nowhere before its new end (:310-313)
    EXPECT(dc.GetLifetimes().size() == lines - 7 && dc.GetLineVertices().size() == 2 * (lines - 7) && dc.GetLineVerticesOffset() == -1);
    dc.ExpireLines(0.1f);
    EXPECT(dc.GetLifetimes().size() == lines - 7 && dc.GetLineVerticesOffset() == -1);
    dc.ExpireLines(0.1f); // 0.25 - 0.3 < 0: the box leaves, from the front
    EXPECT(dc.GetLifetimes().size() == lines - 19 && dc.GetLineVerticesOffset() == 0);
    for (float l : dc.GetLifetimes()) EXPECT(l > 0.5f);
    dc.ExpireLines(5.0f); // everything
    EXPECT(dc.GetLifetimes().empty() && dc.GetLineVertices().empty() && dc.GetLineVerticesOffset() == -1);
    dc.ExpireLines(1.0f);
    for (int round = 0; round < 50; round++) { // lifetimes in every order: the vertices stay paired with their lifetimes
        for (int k = 0; k < 40; k++) {
            const float life = (float)((k * 7 + round * 3) % 11) * 0.1f, a[3] = { life, 0, 0 }, b[3] = { life, 1, 0 };
            dc.DrawLine(a, b, white, life);
        }
        dc.ExpireLines(0.25f);
        EXPECT(dc.GetLineVertices().size() == 2 * dc.GetLifetimes().size());
        for (size_t i = 0; i < dc.GetLifetimes().size(); i++)
            EXPECT(dc.GetLineVertices()[2 * i].position[0] == dc.GetLineVertices()[2 * i + 1].position[0] && dc.GetLifetimes()[i] >= 0.0f &&
                   dc.GetLifetimes()[i] <= dc.GetLineVertices()[2 * i].position[0]);
        dc.GrowIndices();
    }
    dc.Clear();
    EXPECT(dc.GetLineVertices().empty() && dc.GetCachedIndices().empty());
    printf(failures ? "lines_host_check: %d FAILED\n" : "lines_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
