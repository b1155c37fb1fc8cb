// A stand-alone program over the host rule that picks the shade kernels' plane addressing (sailor_amd/csrc/host_rules.h: shade_planes_fit_32_bits), on
// both sides of 2^32 bytes.  Plain C++, no HIP header, no library:
//
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/shade_addressing_host_check.cpp -o /tmp/shade_addressing_host_check
//   /tmp/shade_addressing_host_check
//
// What the kernels need (shade_body.h, !WIDE): the byte offset of every pixel of a plane of the band -- 16 bytes a pixel, pixel index below fbRowCount x width --
// fits 32 bits, and so does the plane stride in bytes.  The expected values below are that statement worked out by hand in 64-bit integers, and a brute-force
// walk over the last pixel's byte offset in 128-bit arithmetic; neither calls the function under test.
#include "../sailor_amd/csrc/host_rules.h"
#include <cstdio>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

// the statement itself: the last byte of the band's plane and the stride in bytes, in arithmetic that cannot wrap
static bool by_definition(unsigned long long stridePixels, long long rows, long long width)
{
    const unsigned __int128 lastByte = (unsigned __int128)rows * (unsigned __int128)width * 16u - 1u; // of the last pixel
    const unsigned __int128 strideBytes = (unsigned __int128)stridePixels * 16u;
    const unsigned __int128 limit = (unsigned __int128)1 << 32;
    return lastByte < limit && strideBytes < limit;
}

int main()
{
    // ---- the frames of the benchmark: far below ----
    EXPECT(shade_planes_fit_32_bits((size_t)3840 * 2160, 2160, 3840));      // 4K: 133 MB a plane
    EXPECT(shade_planes_fit_32_bits((size_t)7680 * 4320, 4320, 7680));      // 8K: 531 MB
    EXPECT(shade_planes_fit_32_bits((size_t)16 * 16, 16, 16));
    // ---- the plane's last byte on both sides of 2^32: 2^28 pixels is the last size that fits ----
    EXPECT(shade_planes_fit_32_bits(((size_t)1 << 28) - 1, 16384, 16384 - 1));   // 268 419 072 pixels
    EXPECT(shade_planes_fit_32_bits(((size_t)1 << 28) - 1, 8192, 32768 - 1));
    EXPECT(!shade_planes_fit_32_bits((size_t)1 << 28, 16384, 16384));            // stride of exactly 2^32 bytes: the planes' bases no longer differ by 32 bits
    EXPECT(!shade_planes_fit_32_bits(((size_t)1 << 28) + 16384, 16385, 16384));  // one row more
    EXPECT(!shade_planes_fit_32_bits((size_t)1 << 30, 16384, 16384));
    // ---- a padded plane stride of 4 GB and more around a small band: the stride alone decides ----
    EXPECT(!shade_planes_fit_32_bits((size_t)1 << 28, 16, 3840));
    EXPECT(shade_planes_fit_32_bits(((size_t)1 << 28) - 1, 16, 3840));
    EXPECT(!shade_planes_fit_32_bits((size_t)1 << 40, 16, 16));                  // (no wrap in the stride's own arithmetic)
    // ---- a band of a tall frame: the band's rows count, not the frame's ----
    EXPECT(shade_planes_fit_32_bits((size_t)1024 * 65536, 1024, 65536));         // 2^26 pixels of a frame that is itself too large
    // ---- against the definition, around every power-of-two shape whose product is 2^28 ----
    int checked = 0;
    for (int lw = 4; lw <= 24; lw++) {
        const long long w0 = 1ll << lw, r0 = 1ll << (28 - lw);
        for (long long dw = -1; dw <= 1; dw++)
            for (long long dr = -1; dr <= 1; dr++) {
                const long long w = w0 + dw, r = r0 + dr;
                if (w <= 0 || r <= 0 || w > INT32_MAX || r > INT32_MAX) continue;
                for (long long pad = 0; pad <= 2; pad++) {
                    const unsigned long long stride = (unsigned long long)(w * r + pad);   // (the entry points refuse a stride below rows x width)
                    EXPECT(shade_planes_fit_32_bits((size_t)stride, (int32_t)r, (int32_t)w) == by_definition(stride, r, w));
                    checked++;
                }
            }
    }
    EXPECT(checked > 500);
    if (failures == 0) printf("shade_addressing_host_check: ok (%d shapes against the definition)\n", checked);
    return failures != 0;
}
