// What accum.hip (multi-sample frames) and denoise.hip (denoised frames) share: the planes of the accumulator state, the frame check
// of their entry points, and the displayed colour of a mean radiance.  Both files are built with contraction off and restated in
// numpy fp32 by the tests, so the one device function here is the one definition of nmf_accum_resolve's and nmf_denoise_finish's
// rgb_map.
#pragma once
#include "common.hpp"

#include <math.h>

#pragma clang fp contract(off)

namespace accum {

// planes of the state, P 4-byte words each (NMF_ACCUM_PLANES of them), then one int32 per tile
enum { PL_COUNT = 0, PL_LIN = 1, PL_ACC = 4, PL_DEPTH = 5, PL_NORMAL = 6, PL_MAP = 9, PL_M2 = 12, PL_END = 15 };
static_assert(PL_END == NMF_ACCUM_PLANES, "state planes");

inline bool finite_f(float v) { return fabsf(v) <= 3.4028235e38f; }      // (false for a NaN)

inline int check_frame(int32_t H, int32_t W, const char* below, const char* above) {
    NMF_REQUIRE(H >= 1 && W >= 1, NMF_EINVAL, below);
    NMF_REQUIRE((int64_t)H * W <= 2147483647LL, NMF_ERANGE, above);
    return NMF_OK;
}

constexpr float SRGB_LIMIT = 0.0031308f;

__device__ __forceinline__ float srgb(float x, int noclip) {
    // nmf_ray_compose_fwd's formula (modules/tonemap.py:34-55); the power in double, rounded once
    const float o = x > SRGB_LIMIT ? 1.055f * (float)pow((double)fmaxf(x, SRGB_LIMIT), 1.0 / 2.4) - 0.055f : 12.92f * x;
    return noclip ? o : fminf(fmaxf(o, 0.f), 1.f);
}

// one channel of rgb_map: the (tonemapped) mean radiance v over the background bg seen through t = 1 - mean acc
__device__ __forceinline__ float displayed(float v, float t, float bg, int tonemap, int noclip) {
    return (tonemap ? srgb(v, noclip) : v) + t * bg;
}

}  // namespace accum
