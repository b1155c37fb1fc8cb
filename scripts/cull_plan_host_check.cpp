// A stand-alone program over the host-side rules of the cull and the shade that need no device: the cull's plan (sailor_amd/csrc/cull_plan.h: plan_cull,
// band_takes_band_form) on both sides of every threshold, the band rule (host_rules.h) on every band of every frame height up to 80, and the environment
// knob helper.  Plain C++, no HIP header, no library:
//
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/cull_plan_host_check.cpp -o /tmp/cull_plan_host_check
//   /tmp/cull_plan_host_check
//
// The expected values were written by reading the host code as it stood BEFORE plan_cull existed (commit b6244eb, sailor_amd/csrc/light_cull.hip: the line
// beside each row is the line of that file that decides it), not by running the function under test.
#include "../sailor_amd/csrc/cull_plan.h"
#include <cstdio>
#include <cstring>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static CullLayout layout(int W, int H, int r0, int r1, int N)
{
    SailorBand b;
    band_from_rows(H, r0, r1, &b);
    return make_layout(W, H, N, b);
}

struct Row {
    const char* what;
    int W, H, r0, r1, N; // the frame, the band's tile rows, the lights
    uint32_t flags;
    float p00, p11;
    // expected
    int brute, select, splits, bandsPerBlock, lightRoleBlocks, intervals, wide, wideExact, coop, headRows;
    uint32_t heavyMin;
    unsigned prepareGrid, listsX, listsY, cullY;
};

#define BF SAILOR_CULL_BRUTE_FORCE
#define IM SAILOR_CULL_INTERVAL_MASKS
#define BS SAILOR_CULL_BAND_SELECT
#define NS SAILOR_CULL_NO_BAND_SELECT

// 640 x 360: Tx 40, Ty 23, groupsX 10; whole frame: 920 tiles, 6 group rows, 16 bands, 2 strips x 23 rows = 46 set-up blocks, 4 frustum blocks,
// head rows (16 * 96 + 9) / 10 = 154.  Tile rows 8..16: 320 tiles, 2 group rows, 12 bands, 16 set-up blocks, 2 frustum blocks.
// H = 16: one tile row, so groupsY = 1 and numBands = groupsX + 1.
static const Row rows[] = {
    // ---- brute: the flag, the perspective gate, N < 512 (:1671-1672); its grid (:1748); prepare's grid (:1715-1727, :1736) ----
    { "n 511",             640, 360, 0, 23, 511, 0, 1.0f, 1.0f,            1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "n 512",             640, 360, 0, 23, 512, 0, 1.0f, 1.0f,            0, 0, 1, 16, 2, 0, 0, 0, 1, 154, 512, 52, 10, 6, 177 },
    { "flag",              640, 360, 0, 23, 512, BF, 1.0f, 1.0f,           1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "flag + intervals",  640, 360, 0, 23, 511, IM, 1.0f, 1.0f,           1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "p00 0.98e-2",       640, 360, 0, 23, 512, 0, 0.98e-2f, 1.0f,        1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "p00 1.02e-2",       640, 360, 0, 23, 512, 0, 1.02e-2f, 1.0f,        0, 0, 1, 16, 2, 0, 0, 0, 1, 154, 512, 52, 10, 6, 177 },
    { "p11 0.98e-2",       640, 360, 0, 23, 512, 0, 1.0f, 0.98e-2f,        1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "p11 1.02e-2",       640, 360, 0, 23, 512, 0, 1.0f, 1.02e-2f,        0, 0, 1, 16, 2, 0, 0, 0, 1, 154, 512, 52, 10, 6, 177 },
    { "p00 1e4",           640, 360, 0, 23, 512, 0, 1e4f, 1.0f,            1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "p00 9999",          640, 360, 0, 23, 512, 0, 9999.0f, 1.0f,         0, 0, 1, 16, 2, 0, 0, 0, 1, 154, 512, 52, 10, 6, 177 },
    { "p11 1e4",           640, 360, 0, 23, 512, 0, 1.0f, 1e4f,            1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    { "p11 -9999 (fabsf)", 640, 360, 0, 23, 512, 0, 1.0f, -9999.0f,        0, 0, 1, 16, 2, 0, 0, 0, 1, 154, 512, 52, 10, 6, 177 },
    { "p00 -0.98e-2",      640, 360, 0, 23, 512, 0, -0.98e-2f, 1.0f,       1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 52, 0, 0, 23 },
    // ---- select: a band, the two flags, N >= 131072 (:1693); 131071 / 131072 lights are 512 light blocks and 2048 words ----
    { "band 131071",       640, 360, 8, 16, 131071, 0, 1.0f, 1.0f,         0, 0, 1, 12, 512, 0, 0, 0, 1, 154, 384, 530, 10, 2, 162 },
    { "band 131072",       640, 360, 8, 16, 131072, 0, 1.0f, 1.0f,         0, 1, 1, 12, 512, 0, 0, 0, 1, 154, 384, 530, 10, 2, 162 },
    { "frame 131072",      640, 360, 0, 23, 131072, 0, 1.0f, 1.0f,         0, 0, 1, 16, 512, 0, 0, 0, 1, 154, 512, 562, 10, 6, 177 },
    { "band 131072 off",   640, 360, 8, 16, 131072, NS, 1.0f, 1.0f,        0, 0, 1, 12, 512, 0, 0, 0, 1, 154, 384, 530, 10, 2, 162 },
    { "band 131071 on",    640, 360, 8, 16, 131071, BS, 1.0f, 1.0f,        0, 1, 1, 12, 512, 0, 0, 0, 1, 154, 384, 530, 10, 2, 162 },
    { "band 600 on",       640, 360, 8, 16, 600, BS, 1.0f, 1.0f,           0, 1, 1, 12, 3, 0, 0, 0, 1, 154, 384, 21, 10, 2, 162 },
    { "band 600 on + off", 640, 360, 8, 16, 600, BS | NS, 1.0f, 1.0f,      0, 0, 1, 12, 3, 0, 0, 0, 1, 154, 384, 21, 10, 2, 162 },
    { "frame 600 on",      640, 360, 0, 23, 600, BS, 1.0f, 1.0f,           0, 0, 1, 16, 3, 0, 0, 0, 1, 154, 512, 53, 10, 6, 177 },
    { "band 511 on",       640, 360, 8, 16, 511, BS, 1.0f, 1.0f,           1, 0, 1, 0, 2, 0, 0, 0, 0, 0, 0, 20, 0, 0, 8 },
    { "band 131072 brute", 640, 360, 8, 16, 131072, BF, 1.0f, 1.0f,        1, 0, 1, 0, 512, 0, 0, 0, 0, 0, 0, 530, 0, 0, 8 },
    // ---- lightBlocks 1023 / 1024: all bands in one block, and the interval masks (:1719-1724) ----
    { "1023 light blocks", 640, 360, 0, 23, 261888, 0, 1.0f, 1.0f,         0, 0, 1, 16, 1023, 0, 0, 0, 1, 154, 512, 1073, 10, 6, 177 },
    { "1024 light blocks", 640, 360, 0, 23, 261889, 0, 1.0f, 1.0f,         0, 0, 1, 16, 1024, 1, 0, 0, 1, 154, 512, 1074, 10, 6, 177 },
    { "intervals flag",    640, 360, 0, 23, 512, IM, 1.0f, 1.0f,           0, 0, 1, 16, 2, 1, 0, 0, 1, 154, 512, 52, 10, 6, 177 },
    // ---- numBands 24 / 25 / 27 (BANDS_PER_BLOCK) and 256 / 257 (MAX_BANDS_PER_BLOCK): splits, the even spread, splits == 1 as the gate on intervals (:1719-1724) ----
    { "24 bands",          1472, 16, 0, 1, 512, 0, 1.0f, 1.0f,             0, 0, 1, 24, 2, 0, 0, 0, 1, 67, 512, 6, 23, 1, 68 },
    { "25 bands",          1536, 16, 0, 1, 512, 0, 1.0f, 1.0f,             0, 0, 2, 13, 4, 0, 0, 0, 1, 64, 512, 8, 24, 1, 65 },
    { "25 bands intervals", 1536, 16, 0, 1, 512, IM, 1.0f, 1.0f,           0, 0, 1, 25, 2, 1, 0, 0, 1, 64, 512, 6, 24, 1, 65 },
    { "27 bands",          1664, 16, 0, 1, 512, 0, 1.0f, 1.0f,             0, 0, 2, 14, 4, 0, 0, 0, 1, 60, 512, 9, 26, 1, 61 },
    { "256 bands",         16320, 16, 0, 1, 512, 0, 1.0f, 1.0f,            0, 0, 11, 24, 22, 0, 0, 0, 1, 7, 512, 58, 255, 1, 8 },
    { "256 bands intervals", 16320, 16, 0, 1, 512, IM, 1.0f, 1.0f,         0, 0, 1, 256, 2, 1, 0, 0, 1, 7, 512, 38, 255, 1, 8 },
    { "257 bands intervals", 16384, 16, 0, 1, 512, IM, 1.0f, 1.0f,         0, 0, 2, 129, 4, 0, 0, 0, 1, 6, 512, 40, 256, 1, 7 },
    // ---- words 4094 / 4096 / 4097 / 4098 / 4608: wide from 4096 even words (:1751), EXACT at a multiple of 512 without the selection (:1756), its grid (:1755),
    //      coop = !wide (:1770), head rows only beside k1_group_lists (:1766, :1771) ----
    { "4094 words",        640, 360, 0, 23, 4094 * 64, 0, 1.0f, 1.0f,      0, 0, 1, 16, 1024, 1, 0, 0, 1, 154, 512, 1074, 10, 6, 177 },
    { "4096 words",        640, 360, 0, 23, 4096 * 64, 0, 1.0f, 1.0f,      0, 0, 1, 16, 1024, 1, 1, 1, 0, 0, 0, 1074, 18, 1, 23 },
    { "4097 words",        640, 360, 0, 23, 4097 * 64, 0, 1.0f, 1.0f,      0, 0, 1, 16, 1025, 1, 0, 0, 1, 154, 512, 1075, 10, 6, 177 },
    { "4098 words",        640, 360, 0, 23, 4098 * 64, 0, 1.0f, 1.0f,      0, 0, 1, 16, 1025, 1, 1, 0, 0, 0, 0, 1075, 18, 1, 23 },
    { "4608 words",        640, 360, 0, 23, 4608 * 64, 0, 1.0f, 1.0f,      0, 0, 1, 16, 1152, 1, 1, 1, 0, 0, 0, 1202, 18, 1, 23 },
    { "4608 words, band",  640, 360, 8, 16, 4608 * 64, 0, 1.0f, 1.0f,      0, 1, 1, 12, 1152, 1, 1, 0, 0, 0, 0, 1170, 6, 1, 8 },
    { "4608, band, off",   640, 360, 8, 16, 4608 * 64, NS, 1.0f, 1.0f,     0, 0, 1, 12, 1152, 1, 1, 1, 0, 0, 0, 1170, 6, 1, 8 },
    { "4095 * 64 + 1",     640, 360, 0, 23, 4095 * 64 + 1, 0, 1.0f, 1.0f,  0, 0, 1, 16, 1024, 1, 1, 1, 0, 0, 0, 1074, 18, 1, 23 },
    // ---- the heavy threshold: bandRows * 2 > Ty (:1765) ----
    { "11 of 23 rows",     640, 360, 0, 11, 512, 0, 1.0f, 1.0f,            0, 0, 1, 13, 2, 0, 0, 0, 1, 154, 384, 26, 10, 3, 165 },
    { "12 of 23 rows",     640, 360, 0, 12, 512, 0, 1.0f, 1.0f,            0, 0, 1, 13, 2, 0, 0, 0, 1, 154, 512, 28, 10, 3, 166 },
    { "12 of 24 rows",     640, 384, 0, 12, 512, 0, 1.0f, 1.0f,            0, 0, 1, 13, 2, 0, 0, 0, 1, 154, 384, 28, 10, 3, 166 },
    { "13 of 24 rows",     640, 384, 11, 24, 512, 0, 1.0f, 1.0f,           0, 0, 1, 14, 2, 0, 0, 0, 1, 154, 512, 31, 10, 4, 167 },
};

// The parent's band test (light_cull.hip:1564-1574 of commit b6244eb), restated: the new rule must give its verdict on every band tried below.
static bool parent_band_valid(int H, const SailorBand* b)
{
    if (!b) return false;
    const int Ty = (H - 1) / TILE + 1;
    if (b->tileRowBegin < 0 || b->tileRowEnd > Ty || b->tileRowBegin > b->tileRowEnd) return false;
    int lo = H - TILE * b->tileRowEnd, hi = H - TILE * b->tileRowBegin;
    if (lo < 0) lo = 0;
    if (hi > H) hi = H;
    if (hi < lo) hi = lo;
    return b->fbRowBegin == lo && b->fbRowCount == hi - lo;
}

int main()
{
    // ---- the plan ----
    for (const Row& r : rows) {
        const CullLayout L = layout(r.W, r.H, r.r0, r.r1, r.N);
        const CullPlan P = plan_cull(L, r.N, r.flags, r.p00, r.p11);
        const bool ok = P.brute == (r.brute != 0) && P.select == (r.select != 0) && P.splits == r.splits && P.bandsPerBlock == r.bandsPerBlock &&
                        P.lightRoleBlocks == r.lightRoleBlocks && P.intervals == (r.intervals != 0) && P.wide == (r.wide != 0) && P.wideExact == (r.wideExact != 0) &&
                        P.coop == (r.coop != 0) && P.headRows == r.headRows && P.heavyMin == r.heavyMin && P.prepareGrid == r.prepareGrid &&
                        P.listsGridX == r.listsX && P.listsGridY == r.listsY && P.cullGridY == r.cullY;
        if (!ok) {
            printf("FAILED row '%s': brute %d select %d splits %d bandsPerBlock %d lightRoleBlocks %d intervals %d wide %d wideExact %d coop %d headRows %d heavyMin %u "
                   "prepareGrid %u lists %u x %u cullY %u\n", r.what, P.brute, P.select, P.splits, P.bandsPerBlock, P.lightRoleBlocks, P.intervals, P.wide, P.wideExact, P.coop,
                   P.headRows, P.heavyMin, P.prepareGrid, P.listsGridX, P.listsGridY, P.cullGridY);
            failures++;
        }
        // what every row shares: one block per 256 lights, the light role's blocks, the parts of prepare's grid (:1715, :1722, :1725-1727, :1736), the tile
        // cull's columns (:1748, :1771), one selection block per 1024 lights (:1706), numBands = 0 under brute force (:1716)
        EXPECT(P.lightBlocks == (r.N + 255) / 256 && P.lightRoleBlocks == P.lightBlocks * P.splits);
        EXPECT(P.prepareGrid == (unsigned)(P.lightRoleBlocks + P.frustumBlocks + P.setupBlocks));
        EXPECT(P.setupBlocks == P.stripsPerRow * L.bandRows && P.frustumBlocks == (L.bandTiles + 255) / 256);
        EXPECT(P.cullGridX == (unsigned)L.groupsX && P.selectGrid == (unsigned)((r.N + 1023) / 1024));
        EXPECT(P.numBands == (r.brute ? 0 : L.numBands));
    }

    // ---- the band form (:1588-1594): a band, <= 12 000 tiles or a set below the large one; SAILOR_BAND_FORM_TILES overrides both ----
    {
        const CullLayout t12000 = layout(3840, 960, 0, 50, 1000), t12001 = layout(17456, 960, 0, 11, 1000), small = layout(640, 360, 8, 16, 1000);
        const CullLayout whole = layout(640, 360, 0, 23, 1000), empty = layout(640, 360, 8, 8, 1000);
        EXPECT(t12000.bandTiles == 12000 && t12001.bandTiles == 12001 && small.bandTiles == 320 && empty.bandTiles == 0);
        EXPECT(band_takes_band_form(t12000, 131071, -1) && band_takes_band_form(t12000, 131072, -1) && band_takes_band_form(t12000, 1000000, -1));
        EXPECT(band_takes_band_form(t12001, 131071, -1) && !band_takes_band_form(t12001, 131072, -1) && !band_takes_band_form(t12001, 1000000, -1));
        EXPECT(!band_takes_band_form(whole, 1000, -1) && !band_takes_band_form(whole, 1000, 100000) && !band_takes_band_form(empty, 1000, -1) &&
               !band_takes_band_form(empty, 1000, 5));
        EXPECT(!band_takes_band_form(small, 1000, 0) && !band_takes_band_form(t12000, 1000, 0));
        EXPECT(band_takes_band_form(small, 1000, 320) && !band_takes_band_form(small, 1000, 319));
        EXPECT(band_takes_band_form(t12001, 131072, 20000) && !band_takes_band_form(t12000, 1000, 11999));
        EXPECT(LARGE_LIGHT_SET == 131072 && BAND_FORM_MAX_TILES == 12000);
    }

    // ---- the knobs: read, range, message ----
    {
        std::string err;
        EXPECT(env_knob(EnvKnob { false, -1 }, 1, 128, &err, "m") == -1 && err.empty());
        EXPECT(env_knob(EnvKnob { true, 1 }, 1, 128, &err, "m") == 1 && env_knob(EnvKnob { true, 128 }, 1, 128, &err, "m") == 128 && err.empty());
        EXPECT(env_knob(EnvKnob { true, 0 }, 1, 128, &err, "m") == -1 && err == "m");
        err.clear();
        EXPECT(env_knob(EnvKnob { true, 129 }, 1, 128, &err, "m") == -1 && err == "m");
        err.clear();
        EXPECT(env_knob(EnvKnob { true, -1 }, 0, 100, &err, "m") == -1 && err == "m");   // set to something atoi reads as -1: out of range, not "unset"
        EXPECT(env_knob(EnvKnob { true, -5 }, 0, INT_MAX, nullptr, nullptr) == -1 && env_knob(EnvKnob { true, 0 }, 0, INT_MAX, nullptr, nullptr) == 0);
        unsetenv("SAILOR_BAND_FORM_TILES");
        EnvKnob k = env_knob_read("SAILOR_BAND_FORM_TILES");
        EXPECT(!k.set && env_knob(k, 0, INT_MAX, nullptr, nullptr) == -1);
        setenv("SAILOR_BAND_FORM_TILES", "0", 1);
        k = env_knob_read("SAILOR_BAND_FORM_TILES");
        EXPECT(k.set && env_knob(k, 0, INT_MAX, nullptr, nullptr) == 0 && !band_takes_band_form(layout(640, 360, 8, 16, 1000), 1000, env_knob(k, 0, INT_MAX, nullptr, nullptr)));
        setenv("SAILOR_BAND_FORM_TILES", "320", 1);
        k = env_knob_read("SAILOR_BAND_FORM_TILES");
        EXPECT(k.set && env_knob(k, 0, INT_MAX, nullptr, nullptr) == 320 && band_takes_band_form(layout(640, 360, 8, 16, 1000), 1000, env_knob(k, 0, INT_MAX, nullptr, nullptr)));
    }

    // ---- the band rule: what band_from_rows builds is valid, and no field of it may move ----
    long bands = 0;
    for (int H = 1; H <= 80; H++) {
        const int Ty = tile_rows_of(H);
        EXPECT(Ty == (H + 15) / 16);
        for (int r0 = 0; r0 <= Ty; r0++)
            for (int r1 = r0; r1 <= Ty; r1++) {
                SailorBand b;
                band_from_rows(H, r0, r1, &b);
                EXPECT(band_is_valid(H, &b) && parent_band_valid(H, &b));
                EXPECT(b.fbRowBegin >= 0 && b.fbRowCount >= 0 && b.fbRowBegin + b.fbRowCount <= H);
                for (int field = 0; field < 4; field++)
                    for (int d = -1; d <= 1; d += 2) {
                        SailorBand m = b;
                        (field == 0 ? m.tileRowBegin : field == 1 ? m.tileRowEnd : field == 2 ? m.fbRowBegin : m.fbRowCount) += d;
                        EXPECT(!band_is_valid(H, &m) && !parent_band_valid(H, &m));
                    }
                SailorBand whole;
                EXPECT(band_or_whole_frame(H, &b, &whole) == &b);
                b.fbRowCount++;
                EXPECT(band_or_whole_frame(H, &b, &whole) == nullptr);
                bands++;
            }
        SailorBand whole;
        EXPECT(band_or_whole_frame(H, nullptr, &whole) == &whole && whole.tileRowBegin == 0 && whole.tileRowEnd == Ty && whole.fbRowBegin == 0 && whole.fbRowCount == H);
        EXPECT(!band_is_valid(H, nullptr));
    }
    if (failures) printf("cull_plan_host_check: %d FAILED\n", failures);
    else printf("cull_plan_host_check: ok (%d plan rows, %ld bands)\n", (int)(sizeof rows / sizeof rows[0]), bands);
    return failures ? 1 : 0;
}
