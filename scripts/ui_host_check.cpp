// A stand-alone program over the host-side logic the RenderImGui pass added: sailor_host_ui_flatten (sailor_amd/csrc/host_math.cpp, compiled INTO this program so
// that the sanitizers see it) over hand-made and random draw data -- hostile values included: NaN and infinite rectangles, sizes and scales, lists whose command
// runs leave the array, offsets that overflow --, the draw-data carrier of the runtime mirror (RHIImGuiDrawData, Runtime/RHI/SceneView.h) filled and flattened the
// way RenderImGuiNode does, and every refusal of sailor_hip_ui_draw / sailor_hip_ui_workspace_bytes (argument checks, the command ranges, the scissors, the
// workspace's size arithmetic).  No GPU is needed or used: every call of the library is refused before anything is launched.
//
//   cd sailor_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I. ../../scripts/ui_host_check.cpp -o /tmp/ui_host_check -L. -lsailor_hip -Wl,-rpath,$PWD && /tmp/ui_host_check
#include "../sailor_amd/csrc/ui_draw.hip"
#include "../sailor_amd/csrc/host_math.cpp"
#include "../sailor_amd/runtime/Runtime/RHI/SceneView.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

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

alignas(16) static char fake[64]; // device pointers are never dereferenced on the host: aligned fakes
static const SailorVertexP2UV2C1* const v = reinterpret_cast<const SailorVertexP2UV2C1*>(fake);
static const SailorUiCommand* const dc = reinterpret_cast<const SailorUiCommand*>(fake);
static float* const target = reinterpret_cast<float*>(fake);

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static float rndf(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xFFFF) / 65535.0f; }

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- sailor_host_ui_flatten ----
    {
        const float pos[2] = { 0, 0 }, size[2] = { 72, 70 }, one[2] = { 1, 1 };
        SailorUiDrawCmd cmds[6] = {};
        const float rects[6][4] = { { -4, -7, 500, 600 }, { 3.7f, 2.2f, 9.2f, 30.9f }, { 10, 10, 10, 20 }, { 70.5f, 60.5f, 80, 90 }, { 0, 0, 0, 0 }, { nan, 0, 5, 5 } };
        for (int k = 0; k < 6; k++) { memcpy(cmds[k].clipRect, rects[k], 16); cmds[k].elemCount = 6; cmds[k].idxOffset = 6u * k; }
        cmds[4].callback = SAILOR_UI_CALLBACK_USER;
        SailorUiDrawList lists[2] = { { 8, 18, 0, 3 }, { 12, 18, 3, 3 } };
        float pc[4];
        SailorUiCommand out[6];
        uint32_t n = 99;
        int32_t w = 0, h = 0;
        EXPECT(sailor_host_ui_flatten(pos, size, one, lists, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_OK && n == 3 && w == 72 && h == 70);
        EXPECT(out[0].scissor[0] == 0 && out[0].scissor[1] == 0 && out[0].scissor[2] == 72 && out[0].scissor[3] == 70);
        EXPECT(out[1].scissor[0] == 3 && out[1].scissor[1] == 2 && out[1].scissor[2] == 5 && out[1].scissor[3] == 28); // the truncated difference, not 6 and 28
        EXPECT(out[2].scissor[0] == 70 && out[2].scissor[1] == 60 && out[2].scissor[2] == 1 && out[2].scissor[3] == 9);
        EXPECT(out[2].firstIndex == 18u + 18u && out[2].vertexOffset == 8 && out[1].firstIndex == 6 && out[1].vertexOffset == 0);
        EXPECT(pc[0] == 2.0f / 72.0f && pc[1] == 2.0f / 70.0f && pc[2] == -1.0f && pc[3] == -1.0f);
        // counting only, and a buffer that is too short
        EXPECT(sailor_host_ui_flatten(pos, size, one, lists, 2, cmds, 6, pc, nullptr, 0, &n, nullptr, nullptr) == SAILOR_HIP_OK && n == 3);
        SailorUiCommand two[2];
        EXPECT(sailor_host_ui_flatten(pos, size, one, lists, 2, cmds, 6, pc, two, 2, &n, &w, &h) == SAILOR_HIP_OK && n == 3);
        // a minimised window, hostile sizes, a list whose run leaves the array, offsets that overflow
        const float tiny[2] = { 0.5f, 70 }, huge[2] = { 3.0e9f, 70 }, bad[2] = { nan, 70 }, neg[2] = { -inf, 70 };
        EXPECT(sailor_host_ui_flatten(pos, tiny, one, lists, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_OK && n == 0 && w == 0);
        EXPECT(sailor_host_ui_flatten(pos, huge, one, lists, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT && n == 0);
        EXPECT(sailor_host_ui_flatten(pos, bad, one, lists, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(sailor_host_ui_flatten(pos, neg, one, lists, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        SailorUiDrawList past[1] = { { 8, 18, 4, 3 } };
        EXPECT(sailor_host_ui_flatten(pos, size, one, past, 1, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        SailorUiDrawList wide[2] = { { 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 1 }, { 4, 6, 1, 1 } };
        EXPECT(sailor_host_ui_flatten(pos, size, one, wide, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(sailor_host_ui_flatten(nullptr, size, one, lists, 2, cmds, 6, pc, out, 6, &n, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(sailor_host_ui_flatten(pos, size, one, lists, 2, cmds, 6, pc, out, 6, nullptr, &w, &h) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(sailor_host_ui_flatten(pos, size, one, nullptr, 0, nullptr, 0, pc, out, 6, &n, &w, &h) == SAILOR_HIP_OK && n == 0);
    }
    // ---- the mirror's carrier, filled at random and flattened as RenderImGuiNode does; every scissor must lie inside the framebuffer ----
    for (int round = 0; round < 2000; round++) {
        Sailor::RHI::RHIImGuiDrawData ui;
        const float special[6] = { nan, inf, -inf, 0.0f, -0.0f, 1.0e30f };
        auto value = [&](float lo, float hi) { return (rnd() % 23u) == 0u ? special[rnd() % 6u] : rndf(lo, hi); };
        for (int k = 0; k < 2; k++) { ui.m_displayPos[k] = value(-100, 100); ui.m_displaySize[k] = value(0, 300); ui.m_framebufferScale[k] = value(0.5f, 2.5f); }
        const uint32_t numLists = rnd() % 4u;
        for (uint32_t l = 0; l < numLists; l++) {
            SailorUiDrawList list = { rnd() % 50u, rnd() % 90u, (uint32_t)ui.m_cmds.size(), rnd() % 5u };
            for (uint32_t c = 0; c < list.cmdCount; c++) {
                SailorUiDrawCmd cmd = {};
                for (int k = 0; k < 4; k++) cmd.clipRect[k] = value(-150, 450);
                cmd.elemCount = rnd() % 40u; cmd.idxOffset = rnd() % 90u; cmd.vtxOffset = rnd() % 50u; cmd.callback = rnd() % 4u;
                ui.m_cmds.push_back(cmd);
            }
            ui.m_lists.push_back(list);
            ui.m_vertices.resize(ui.m_vertices.size() + list.vtxCount);
            ui.m_indices.resize(ui.m_indices.size() + list.idxCount);
        }
        float pc[4];
        uint32_t count = 0;
        int32_t width = 0, height = 0;
        std::vector<SailorUiCommand> flat(ui.m_cmds.size() ? ui.m_cmds.size() : 1);
        const int st = sailor_host_ui_flatten(ui.m_displayPos, ui.m_displaySize, ui.m_framebufferScale, ui.m_lists.data(), (uint32_t)ui.m_lists.size(), ui.m_cmds.data(),
                                              (uint32_t)ui.m_cmds.size(), pc, flat.data(), (uint32_t)flat.size(), &count, &width, &height);
        if (st != SAILOR_HIP_OK) { EXPECT(count == 0); continue; }
        EXPECT(count <= ui.m_cmds.size());
        for (uint32_t i = 0; i < count; i++) {
            const SailorUiCommand& c = flat[i];
            EXPECT(c.scissor[0] >= 0 && c.scissor[1] >= 0 && c.scissor[2] >= 0 && c.scissor[3] >= 0);
            EXPECT((long long)c.scissor[0] + c.scissor[2] <= width && (long long)c.scissor[1] + c.scissor[3] <= height);
        }
    }
    // ---- the refusals of the entry points ----
    {
        SailorHipContext ctx;
        const int32_t W = 72, H = 70;
        SailorBand band, bad, none;
        sailor_hip_band_whole_frame(W, H, &band);
        bad = band; bad.fbRowCount = H + 1;
        none = band; none.tileRowBegin = none.tileRowEnd; none.fbRowBegin = H - 16 * none.tileRowEnd < 0 ? 0 : H - 16 * none.tileRowEnd; none.fbRowCount = 0;
        size_t bytes = 7;
        EXPECT(sailor_hip_ui_workspace_bytes(2, W, H, nullptr) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(sailor_hip_ui_workspace_bytes(2, 0, H, &bytes) == SAILOR_HIP_ERR_INVALID_ARGUMENT && bytes == 0);
        EXPECT(sailor_hip_ui_workspace_bytes(2, W, H, &bytes) == SAILOR_HIP_OK && bytes == UI_HEADER_BYTES + 160);
        size_t most = 0;
        EXPECT(sailor_hip_ui_workspace_bytes(0xFFFFFFFFu, W, H, &most) == SAILOR_HIP_OK && most == UI_HEADER_BYTES + 80ull * 0xFFFFFFFFull);
        const float scale[2] = { 2.0f / W, 2.0f / H }, translate[2] = { -1, -1 };
        SailorTextureDesc tex = {};
        SailorUiCommand good = { 0, 6, 0, { 0, 0, W, H } };
        auto draw = [&](const SailorUiCommand& c, uint32_t indexBytes = 2, uint32_t numIndices = 6, const void* idx = fake, const SailorVertexP2UV2C1* vb = v,
                        const SailorUiCommand* dcmd = dc, void* ws = fake, size_t n = 0, float* t = target, int32_t w = W, const SailorBand* b = nullptr,
                        const SailorTextureDesc* tx = nullptr, uint32_t numCommands = 1) {
            return sailor_hip_ui_draw(&ctx, vb, 4, idx, indexBytes, numIndices, &c, dcmd, numCommands, scale, translate, tx ? tx : &tex, ws, n ? n : bytes, t, w, H,
                                      b ? b : &band);
        };
        EXPECT(sailor_hip_ui_draw(nullptr, v, 4, fake, 2, 6, &good, dc, 1, scale, translate, &tex, fake, bytes, target, W, H, &band) == SAILOR_HIP_ERR_INVALID_ARGUMENT);
        EXPECT(refused(ctx, draw(good, 3), "index width"));
        EXPECT(refused(ctx, draw(good, 2, 5), "index range"));
        EXPECT(refused(ctx, draw(good, 2, 6, nullptr), "index buffer"));
        EXPECT(refused(ctx, draw(good, 4, 6, fake + 2), "index buffer"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, nullptr), "vertex buffer"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, reinterpret_cast<const SailorVertexP2UV2C1*>(fake + 2)), "vertex buffer"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, nullptr), "command array"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, nullptr), "workspace is NULL"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake + 8), "16-byte aligned"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes - 1), "smaller than"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, nullptr), "the target"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, reinterpret_cast<float*>(fake + 4)), "the target"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, target, 0), "extent"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, target, W, &bad), "band"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, target, W, &band, nullptr, SAILOR_UI_MAX_COMMANDS + 1), "SAILOR_UI_MAX_COMMANDS"));
        SailorTextureDesc srgb = { reinterpret_cast<const uint32_t*>(fake), 8, 8, SAILOR_TEXTURE_SRGB, 0 }, odd = { reinterpret_cast<const uint32_t*>(fake + 2), 8, 8, 0, 0 };
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, target, W, &band, &srgb), "sRGB"));
        EXPECT(refused(ctx, draw(good, 2, 6, fake, v, dc, fake, bytes, target, W, &band, &odd), "texels"));
        const int32_t scissors[7][4] = { { -1, 0, 5, 5 }, { 0, -1, 5, 5 }, { 0, 0, -1, 5 }, { 0, 0, 5, -1 }, { W - 4, 0, 5, 5 }, { 0, H - 4, 5, 5 },
                                         { 0x7FFFFFFF, 0, 0x7FFFFFFF, 1 } };
        for (auto& s : scissors) {
            SailorUiCommand c = good;
            memcpy(c.scissor, s, 16);
            EXPECT(refused(ctx, draw(c), "scissor"));
        }
        SailorUiCommand far = good;
        far.firstIndex = 0xFFFFFFFFu; far.indexCount = 0xFFFFFFFFu; // the sum needs 64 bits
        EXPECT(refused(ctx, draw(far), "index range"));
        SailorUiCommand empty = good;
        empty.indexCount = 2; // no whole triangle: accepted, records nothing, and needs neither buffer
        EXPECT(draw(empty, 2, 6, nullptr, nullptr) == SAILOR_HIP_OK && ctx.launchCount == 0);
        EXPECT(draw(good, 2, 6, fake, v, dc, fake, bytes, nullptr, W, &none) == SAILOR_HIP_OK && ctx.launchCount == 0); // a band without rows has no target
        EXPECT(sailor_hip_ui_draw(&ctx, nullptr, 0, nullptr, 2, 0, nullptr, nullptr, 0, scale, translate, &tex, fake, bytes, target, W, H, &band) == SAILOR_HIP_OK &&
               ctx.launchCount == 0); // no commands
    }
    printf(failures ? "ui_host_check: %d FAILED\n" : "ui_host_check: ok%.0d\n", failures);
    return failures ? 1 : 0;
}
