// Motion-compensated temporal denoising in integers (lfg_denoise_temporal, include/linuxfg_hip.h):
// what a pixel does once the window costs of its references are known -- the weights, their normalisation to 256ths, the mix
// and the limit.  Host and device code share this header; it needs nothing but the standard library, so that the kernel
// (denoise.hip) and tests/cpp/denoise_on_host.cpp, built with g++ alone, run the same text.
//
// Ranges (radius <= 2: at most 25 window texels; tolerance <= 1020, strength <= 256): L = tolerance * n <= 25,500, a cost
// <= 25 * 4 * 255 = 25,500, a weight <= (256 * 25,500) >> 6 = 102,000, D = L + w_1 + w_2 <= 229,500, 256 * w <= 26,112,000:
// every intermediate fits 32 bits.  L >= 1, so a_1 + a_2 <= floor(256 (D - L) / D) <= 255 and a_0 >= 1.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define LFG_DENOISE_FN __host__ __device__ inline
#else
#define LFG_DENOISE_FN inline
#endif

namespace lfg {

constexpr int kDenoiseMaxRefs = 2, kDenoiseMaxRadius = 2;
constexpr int kDenoiseMaxTolerance = 1020, kDenoiseMaxStrength = 256, kDenoiseMaxLimit = 255;

// The shares of the mix in 256ths: a[0] curr's, a[1] and a[2] the references'.  They sum to 256 and a[0] >= 1.
struct DenoiseShares { uint32_t a[1 + kDenoiseMaxRefs]; };

// w = (strength * max(0, L - cost)) >> 6, and 0 where the vector points out of the image.
LFG_DENOISE_FN uint32_t denoise_weight(uint32_t strength, uint32_t L, uint32_t cost, bool targetInside) {
    return targetInside && cost < L ? (strength * (L - cost)) >> 6 : 0u;
}

// a_i = floor(256 w_i / D), D = L + w_1 + w_2; a_0 the rest.  An absent second reference has w2 = 0.
LFG_DENOISE_FN DenoiseShares denoise_shares(uint32_t L, uint32_t w1, uint32_t w2) {
    const uint32_t D = L + w1 + w2;
    DenoiseShares s;
    s.a[1] = (256u * w1) / D;
    s.a[2] = (256u * w2) / D;
    s.a[0] = 256u - s.a[1] - s.a[2];
    return s;
}

// One channel: the mix, rounded to nearest, held to curr +- limit.  All values bytes; the result is one.
LFG_DENOISE_FN uint32_t denoise_channel(const DenoiseShares &s, uint32_t c, uint32_t r1, uint32_t r2, uint32_t limit) {
    const int m = (int)((s.a[0] * c + s.a[1] * r1 + s.a[2] * r2 + 128u) >> 8);
    const int lo = (int)c - (int)limit, hi = (int)c + (int)limit;
    return (uint32_t)(m < lo ? lo : (m > hi ? hi : m));
}

// All four channels of a packed texel.  The result of denoise_channel is limited to curr +- limit, not to a constant byte
// range, so this is not the shift-clamp-pack pattern that yuv_convert.hip keeps apart.
LFG_DENOISE_FN uint32_t denoise_texel(const DenoiseShares &s, uint32_t c, uint32_t r1, uint32_t r2, uint32_t limit) {
    uint32_t px = 0u;
    for (int k = 0; k < 32; k += 8)
        px |= denoise_channel(s, (c >> k) & 255u, (r1 >> k) & 255u, (r2 >> k) & 255u, limit) << k;
    return px;
}

}  // namespace lfg
