// The mip chain of a 2-D RGBA8 material texture: what GenerateMipMaps records for every imported texture (TextureAssetInfo.h:34; TextureImporter.cpp:247-295;
// VulkanCommandBuffer.cpp:814-907: level l + 1 is a 2:1 VK_FILTER_LINEAR blit of level l).  include/sailor_hip.h (the mip-mapped section) has the pinned
// rules; tests/lod_ref.py restates them sequentially next to a float64 twin, and the kernel is held to the restatement byte for byte.
//
//   k_texture_mip_down   a lane per texel of the smaller level: decode the four taps (sRGB table for r, g, b under the flag, byte / 255 otherwise), lerp2 with
//                        sailor_hip_blit_linear's taps, encode (sRGB: a binary search of the 255 rounding boundaries; UNORM: floorf(x * 255 + 0.5)).
#include "surface_lod.h"

struct MipEncode { float v[256]; }; // v[k - 1] = the decode of (k - 0.5) / 255; v[255] is never read

// the number of boundaries <= x: the byte whose decode is nearest below
__device__ __forceinline__ uint32_t mip_encode_srgb(const MipEncode& enc, float x)
{
    uint32_t lo = 0, hi = 255;
#pragma unroll 1
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (enc.v[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t mip_encode_unorm(float x) { return (uint32_t)floorf(x * 255.0f + 0.5f); }

__global__ __launch_bounds__(256) void k_texture_mip_down(const uint32_t* __restrict__ src, int SW, int SH, uint32_t* __restrict__ dst, int W, int H, int srgb, SurfSrgb dec,
                                                          MipEncode enc)
{
    const int i = texel_i(), j = texel_j();
    if (i >= W || j >= H) return;
    const float u = ((float)i + 0.5f) / (float)W, v = ((float)j + 0.5f) / (float)H;
    const BilinearTaps t = bilinear_taps(SW, SH, u, v);
    const uint32_t a = src[(size_t)t.y0 * SW + t.x0], c = src[(size_t)t.y0 * SW + t.x1], d = src[(size_t)t.y1 * SW + t.x0], e = src[(size_t)t.y1 * SW + t.x1];
    uint32_t out = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
        const uint32_t ba = (a >> (8 * ch)) & 255u, bc = (c >> (8 * ch)) & 255u, bd = (d >> (8 * ch)) & 255u, be = (e >> (8 * ch)) & 255u;
        uint32_t byte;
        if (srgb && ch < 3) byte = mip_encode_srgb(enc, lerp2(dec.v[ba], dec.v[bc], dec.v[bd], dec.v[be], t.ax, t.ay));
        else byte = mip_encode_unorm(lerp2(unorm8(ba), unorm8(bc), unorm8(bd), unorm8(be), t.ax, t.ay));
        out |= byte << (8 * ch);
    }
    dst[(size_t)j * W + i] = out;
}

extern "C" {

uint32_t sailor_hip_texture_mip_levels(int32_t width, int32_t height)
{
    return extent_ok(width, height) ? (uint32_t)surf_full_levels(width, height) : 0u;
}

int sailor_host_srgb_encode_table(float out[255])
{
    if (!out) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    for (int k = 1; k < 256; k++) {
        const double c = ((double)k - 0.5) / 255.0;
        out[k - 1] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
    }
    return SAILOR_HIP_OK;
}

int sailor_hip_texture_generate_mips(SailorHipContext* ctx, uint32_t* dTexels, int32_t width, int32_t height, uint32_t levels, uint32_t flags)
{
    if (!ctx) return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const char* why = nullptr;
    if (!aligned(dTexels, 4)) why = "the texels are NULL or not 4-byte aligned";
    else if (!extent_ok(width, height)) why = "an extent is outside 1 .. 32768";
    else if (levels < 1u || levels > sailor_hip_texture_mip_levels(width, height)) why = "levels is outside 1 .. floor(log2(max(width, height))) + 1";
    else if (flags & ~SAILOR_TEXTURE_SRGB) why = "unknown flags";
    if (why) return surf_refuse(ctx, "sailor_hip_texture_generate_mips", why);
    if (levels == 1u) return SAILOR_HIP_OK;
    static const SurfSrgb dec = [] { SurfSrgb t; sailor_host_srgb_table(t.v); return t; }();
    static const MipEncode enc = [] { MipEncode t; sailor_host_srgb_encode_table(t.v); t.v[255] = 2.0f; return t; }();
    SAILOR_TRY_HIP(ctx, hipSetDevice(ctx->device));
    for (uint32_t l = 0; l + 1 < levels; l++) {
        const int sw = surf_level_extent(width, (int)l), sh = surf_level_extent(height, (int)l), dw = surf_level_extent(width, (int)l + 1),
                  dh = surf_level_extent(height, (int)l + 1);
        sailor_launch(ctx, k_texture_mip_down, texel_grid(dw, dh), dim3(256), (const uint32_t*)(dTexels + surf_level_offset(width, height, (int)l)), sw, sh,
                      dTexels + surf_level_offset(width, height, (int)l + 1), dw, dh, (flags & SAILOR_TEXTURE_SRGB) ? 1 : 0, dec, enc);
        SAILOR_CHECK_LAUNCH(ctx, "k_texture_mip_down");
    }
    return SAILOR_HIP_OK;
}

} // extern "C"
