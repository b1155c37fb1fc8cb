// What the two routes of the Transparent queue share on the host (surface_transparent.hip: the peel; surface_buckets.hip: the per-pixel buckets): the blend
// field of a draw's flags and MULTIPLY's refusal.  The draw kernels' body is surface_masked_body.h.
#pragma once
#include "surface_masked_body.h"

static const uint32_t PEEL_BLEND_BITS = SAILOR_SURFACE_BLEND_MASK << SAILOR_SURFACE_BLEND_SHIFT;

static bool peel_is_multiply(const SailorSurfaceDraw* draw)
{
    return ((draw->flags >> SAILOR_SURFACE_BLEND_SHIFT) & SAILOR_SURFACE_BLEND_MASK) == SAILOR_SURFACE_BLEND_MULTIPLY;
}
static int peel_refuse_multiply(SailorHipContext* ctx, const char* who)
{
    ctx->lastError = std::string(who) + ": EBlendMode::Multiply is not a blend of scene draws (VK_BLEND_OP_MULTIPLY_EXT)";
    return SAILOR_HIP_ERR_UNSUPPORTED;
}
