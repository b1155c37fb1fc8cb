// K1's host side in plain C++ (no HIP, nothing read from the device): where a cull's sections lie in the workspace (CullLayout) and which kernels a
// cull launches on which grids (CullPlan).  light_cull.hip fills the argument structs and launches from these two and decides nothing itself; a threshold
// is changed HERE, next to the measurement that set it.  scripts/cull_plan_host_check.cpp holds both sides of every threshold, without a device.
#pragma once
#include <math.h>
#include "host_rules.h"

#define BANDS_PER_BLOCK 24   // group columns / rows whose masks one light block of k01_prepare builds when the lights alone do not fill the chip
#define MAX_BANDS_PER_BLOCK 256 // ... and at most (LDS for their planes); with >= 1024 light blocks a block builds all of its lights' masks
#define GROUP 4              // k1_group_lists: tiles per group edge (4x4 tiles share one candidate list)
#define CAPG 2048            // entries per group list; a denser group falls back to walking the masks per tile
// A group with more candidates than this is listed as a light cluster: its tiles get a block each.  Measured 512 / 384 / 256: whole frame 25.5 / 26.1 /
// 30.6 us for k1_tile_cull, a cluster band of an 8-way split 15.4 / 9.7 / 8.0 -- the whole frame hides a long block behind its other 8 000, a band
// IS its longest block; below 384 too many groups qualify.  So: by the size of the band.
#define HEAVY_MIN_FRAME 512
#define HEAVY_MIN_BAND 384
#define HEAVY_MAX 96            // ... and that list's room (16 head blocks of k1_tile_cull per entry: the empty ones are dispatched in front of everything else -- 4 096 of them cost ~3 us)
#define PACK_TILES 64        // tiles per k1_pack block
#define SEL_LIGHTS 1024      // lights per block of k0_band_count / k0_band_scatter
#define SETUP_STRIPS 2       // k1_tile_setup: 16-tile strips per block: the whole role is one round of resident blocks at 4K, 8 float4 loads in flight per lane
#define GLW_ROWS 4           // k1_group_lists_wide: rows of 128 words per step
#define BAND_FORM_MAX_TILES 12000 // (see band_takes_band_form)

struct CullLayout {
    int Tx, Ty, bandRows, bandTiles, numBands, words, groupsX, groupsY, numGroups, packBlocks;
    size_t offLightView, offLightType, offTileInfo, offMasks, offDirWords, offGroupCount, offGroupList, offTileNum, offTileNum8, offTileLists, offDirFlag, offHeavy,
           offLightMap, offSelState, offSelKeep, total;
    int selBlocks;
};

static inline CullLayout make_layout(int W, int H, int N, const SailorBand& band)
{
    CullLayout L;
    L.Tx = (W - 1) / TILE + 1;
    L.Ty = (H - 1) / TILE + 1;
    L.bandRows = band.tileRowEnd - band.tileRowBegin;
    L.bandTiles = L.bandRows * L.Tx;
    L.words = (N + 63) / 64;
    if (L.words < 1) L.words = 1;
    const size_t n = (size_t)(N > 0 ? N : 1);
    const size_t tiles = (size_t)(L.bandTiles > 0 ? L.bandTiles : 1);
    L.groupsX = (L.Tx + GROUP - 1) / GROUP;
    L.groupsY = (L.bandRows + GROUP - 1) / GROUP;
    L.numGroups = L.groupsX * L.groupsY;
    L.numBands = L.groupsX + L.groupsY;      // group columns first, then the band's group rows (4 tiles wide / high)
    L.packBlocks = (L.bandTiles + PACK_TILES - 1) / PACK_TILES;
    const size_t groups = (size_t)(L.numGroups > 0 ? L.numGroups : 1);
    // Sections whose size depends on the geometry only come first, those that scale with the light count last: the offset of anything a later
    // call looks up from (width, height, band) alone -- the per-tile lists, their lengths -- is then the same for every lightsNum <= the capacity the
    // workspace was sized for (a cull may run with fewer lights than the capacity; round 2 computed the hint's address from the capacity and
    // the cull's own layout from lightsNum, which only agree when the two are equal).
    size_t o = 0;
    L.offTileInfo = o; o = align_up(o + tiles * 64, 256);
    L.offGroupCount = o; o = align_up(o + groups * 4, 256);
    L.offDirFlag = o; o = align_up(o + 4, 256);
    L.offHeavy = o; o = align_up(o + (1 + HEAVY_MAX) * 4, 256); // [0] = light-cluster groups listed by k1_group_lists (zeroed by k01_prepare), then their indices
    L.offGroupList = o; o = align_up(o + groups * CAPG * 4, 256);
    L.offTileNum = o; o = align_up(o + tiles * 4, 256);
    L.offTileNum8 = o; o = align_up(o + tiles + 64, 256);      // the same lengths (<= 128) as bytes: what k1_pack adds up for its base (32 KB at 4K instead of 130)
    L.offTileLists = o; o = align_up(o + tiles * KEEP * 4, 256); // one fixed 128-entry slot per tile (only the list's own bytes are ever touched)
    L.offLightView = o; o = align_up(o + n * 16, 256);
    L.offLightType = o; o = align_up(o + n * 4, 256);
    L.offMasks = o; o = align_up(o + (size_t)(L.numBands > 0 ? L.numBands : 1) * L.words * 8, 256);
    L.offDirWords = o; o = align_up(o + (size_t)L.words * 8, 256);
    // the band's own light set (k0_band_count / k0_band_scatter: split frames with large light sets): compact index -> light index; [0] the number of
    // selected lights, [2 + b] block b's count; block b's sixteen ballot words
    L.selBlocks = (int)((n + SEL_LIGHTS - 1) / SEL_LIGHTS);
    L.offLightMap = o; o = align_up(o + n * 4, 256);
    L.offSelState = o; o = align_up(o + (size_t)(2 + L.selBlocks) * 4, 256);
    L.offSelKeep = o; o = align_up(o + (size_t)L.selBlocks * 16 * 8, 256);
    L.total = o;
    return L;
}

// The BAND FORM of the shade (shade.hip: split blocks for the long tiles in front of the one-block-per-tile grid) is what sailor_hip_light_cull_tile_order
// switches on by handing a band's per-tile list lengths to the shade.  Every band of a split frame gets it -- the split threshold rises with the band's
// size (shade_body.h: SPLIT_MIN_*) -- but a band of more than BAND_FORM_MAX_TILES tiles under a LARGE light set (LARGE_LIGHT_SET: an eighth of the
// 8K frame under a million lights, 16 320 tiles): such a set means short lists and next to no long tiles (225 of 16 320 there), so there is no tail to cut,
// and the band takes the whole frame's form -- one block per tile on the XCD-aware grid -- whose launch pipelines better beside the next frame's cull
// (step 116.5 against 126.3 us, same box; the 4K frame's halves under 65 536 lights: 103.2 / 95.7 us in the band form, 108.0 / 91.9 in the other).
// `limit` = SAILOR_BAND_FORM_TILES=<n>, which overrides the limit (A / B; 0: never the band form), or -1: not set.
static inline bool band_takes_band_form(const CullLayout& L, const int lightsCapacity, const int limit)
{
    if (L.bandRows >= L.Ty || L.bandTiles <= 0) return false; // whole frame: the one-block-per-tile form in raster order
    if (limit >= 0) return L.bandTiles <= limit;
    return L.bandTiles <= BAND_FORM_MAX_TILES || lightsCapacity < LARGE_LIGHT_SET;
}

// Every decision of one cull (sailor_hip_light_cull_prepared), made once.  Launches, in order: [select: k0_band_count, k0_band_scatter on selectGrid,]
// k01_prepare on prepareGrid, then k1_tile_cull_brute on cullGrid (brute) or { k1_group_lists_wide<wideExact> (wide) or k1_group_lists on listsGrid[XY],
// k1_tile_cull<coop, select> on cullGrid }, then k1_pack on L.packBlocks unless the caller defers it.
struct CullPlan {
    bool brute;      // every tile walks every light: no band masks, no group lists
    bool select;     // the band's own light set first; the chain runs on compact indices
    bool intervals;  // band masks by bisection
    bool wide;       // k1_group_lists_wide and the per-wave selection in k1_tile_cull
    bool wideExact;  // ... its instantiation without bounds checks
    bool coop;       // k1_tile_cull's block-wide selection
    int lightBlocks, splits, bandsPerBlock, lightRoleBlocks, numBands; // the light role of k01_prepare (numBands: 0 under brute force)
    int stripsPerRow, setupBlocks, frustumBlocks;                      // its depth and frustum roles
    int headRows;        // k1_tile_cull's grid rows in front of the tile rows: the listed clusters' tiles, a block each
    uint32_t heavyMin;   // k1_group_lists lists a group with more candidates than this as a cluster (0: no cluster list on this path)
    unsigned selectGrid, prepareGrid, listsGridX, listsGridY, cullGridX, cullGridY;
};

static inline CullPlan plan_cull(const CullLayout& L, const int N, const uint32_t flags, const float projection0, const float projection5)
{
    CullPlan P;
    // The side-plane margin argument needs a sane perspective; tiny light counts are cheaper brute force.
    const float p00 = fabsf(projection0), p11 = fabsf(projection5);
    const bool sane = p00 > 1e-2f && p11 > 1e-2f && p00 < 1e4f && p11 < 1e4f;
    P.brute = (flags & SAILOR_CULL_BRUTE_FORCE) || !sane || N < 512;
    // A band of a split frame with a large light set: the lights that can reach the band are selected first (k0_band_count + k0_band_scatter) and the chain runs on them.
    // From LARGE_LIGHT_SET lights on (below, the light role and the group lists of a band sit at their launch floors whatever the count); SAILOR_CULL_BAND_SELECT
    // forces it for any set the pre-filter runs on, SAILOR_CULL_NO_BAND_SELECT switches it off.  (Two launches, no block waits for another: any
    // number of blocks.)
    P.select = !P.brute && L.bandRows < L.Ty && !(flags & SAILOR_CULL_NO_BAND_SELECT) && ((flags & SAILOR_CULL_BAND_SELECT) || N >= LARGE_LIGHT_SET);
    P.selectGrid = (unsigned)L.selBlocks;

    P.lightBlocks = (N + 255) / 256;
    P.numBands = P.brute ? 0 : L.numBands;
    // Few lights: the bands are spread over several blocks per 256 lights (parallelism; every block repeats the cheap transform).  Many lights
    // (the 1 M of configs[4]): the light blocks fill the chip by themselves, and repeating the 112-byte record reads per split is what costs.
    const bool allBands = P.lightBlocks >= 1024 || (flags & SAILOR_CULL_INTERVAL_MASKS);
    const int perBlock = allBands ? MAX_BANDS_PER_BLOCK : BANDS_PER_BLOCK;
    P.splits = P.brute ? 1 : (L.numBands + perBlock - 1) / perBlock;
    P.bandsPerBlock = P.brute ? 0 : (L.numBands + P.splits - 1) / P.splits; // the bands spread evenly over the splits
    P.lightRoleBlocks = P.lightBlocks * P.splits;
    // the masks by bisection for each light's band intervals instead of 2 x numBands plane tests: needs all bands in one block
    P.intervals = !P.brute && P.splits == 1 && allBands;
    P.stripsPerRow = (L.Tx + 16 * SETUP_STRIPS - 1) / (16 * SETUP_STRIPS);
    P.setupBlocks = P.stripsPerRow * L.bandRows;
    P.frustumBlocks = (L.bandTiles + 255) / 256;
    P.prepareGrid = (unsigned)(P.lightRoleBlocks + P.frustumBlocks + P.setupBlocks);

    P.wide = !P.brute && L.words >= 4096 && (L.words & 1) == 0;
    P.wideExact = P.wide && L.words % (128 * GLW_ROWS) == 0 && !P.select;
    // (the block-wide selection everywhere but on the long lists of the wide path: see k1_tile_cull)
    P.coop = !P.brute && !P.wide;
    const bool clusters = !P.brute && !P.wide; // k1_group_lists keeps the cluster list; the wide path has none
    P.heavyMin = clusters ? (uint32_t)(L.bandRows * 2 > L.Ty ? HEAVY_MIN_FRAME : HEAVY_MIN_BAND) : 0u;
    P.headRows = clusters ? (16 * HEAVY_MAX + L.groupsX - 1) / L.groupsX : 0;
    // (round 6: a 4 x 4 patch of groups per block halved the masks' traffic of the wide lists, shortened nothing and slowed the frame pipeline: removed)
    P.listsGridX = P.brute ? 0u : (P.wide ? (unsigned)(((L.groupsX + 3) / 4) * L.groupsY) : (unsigned)L.groupsX);
    P.listsGridY = P.brute ? 0u : (P.wide ? 1u : (unsigned)L.groupsY);
    P.cullGridX = (unsigned)L.groupsX;
    P.cullGridY = (unsigned)(P.headRows + L.bandRows);
    return P;
}
