// The bicubic fetch of the compensated routes in integers (lfg_interpolate_compensated_sampled, include/linuxfg_hip.h;
// DESIGN.md section 4.23): the weight rule and the body from 16 texel words and two phases to the four 16-bit sample values p.
// Host and device code share this header; it needs nothing but the standard library, so that lfg_sampling_weights
// (lfg_capi.cpp), the sampling kernels (interpolate_bicubic.hip, through lfg_interp.hpp) and tests/cpp/bicubic_on_host.cpp,
// built with g++ alone, all run the same text.
#pragma once

#include <cstdint>

namespace lfg {

constexpr int kBicubicPhases = 64;             // phases per texel: phi = (int)(fraction * 64.0f)
constexpr int kBicubicOne = 16384;             // a row of weights sums to this, exactly
constexpr int kBicubicPMax = 65280;            // p of a texel byte b is 256 b; the fetch clamps p to [0, 256 * 255]

// Catmull-Rom at f = phi / 64 in 14-bit fixed point, from exact integers: the numerators below sum to 2 * 64^3, each weight is
// the floor of (n + 16) / 32, and the tap nearest the position takes what is left of 16384.  phi = 64 is in the rule's reach
// too and gives (0, 16384 at tap 2, 0): the texel one to the right, as phase 0 of the next texel.  The fraction u - floorf(u)
// rounds to 1.0f for a tiny negative u, so a fetch can ask for it; the table lfg_sampling_weights hands out ends at 63.
// Every weight fits 16 bits (-1213 .. 16384); the casts say so to the compiler, which then multiplies in 24 bits.
struct BicubicRow { int w[4]; };
constexpr BicubicRow bicubic_row(int phi) {
    const int p2 = phi * phi, p3 = p2 * phi;
    int w0 = (-4096 * phi + 128 * p2 - p3 + 16) >> 5;
    int w1 = (524288 - 320 * p2 + 3 * p3 + 16) >> 5;
    int w2 = (4096 * phi + 256 * p2 - 3 * p3 + 16) >> 5;
    int w3 = (-64 * p2 + p3 + 16) >> 5;
    if (phi <= 32) w1 = kBicubicOne - w0 - w2 - w3;
    else w2 = kBicubicOne - w0 - w1 - w3;
    return BicubicRow{{(int)(int16_t)w0, (int)(int16_t)w1, (int)(int16_t)w2, (int)(int16_t)w3}};
}

// The phase of a fraction in [0, 1]: truncated, never rounded.
constexpr int bicubic_phase(float fraction) { return (int)(fraction * 64.0f); }

constexpr int bicubic_byte(uint32_t texel, int c) { return (int)((texel >> (8 * c)) & 0xffu); }

// One channel: four horizontal sums h_r = (sum_k wx[k] * texel(r, k) + 64) >> 7 (arithmetic shifts: floors; |h_r| <= 40,800),
// their vertical sum s (|s| <= 835,584,000 < 2^31), and p = clamp((s + 4096) >> 13, 0, 65280).  t[4 * r + k] is texel(r, k).
constexpr int bicubic_channel(const uint32_t (&t)[16], int c, const BicubicRow &wx, const BicubicRow &wy) {
    int s = 0;
    for (int r = 0; r < 4; ++r) {
        int h = 64;
        for (int k = 0; k < 4; ++k) h += wx.w[k] * bicubic_byte(t[4 * r + k], c);
        s += wy.w[r] * (h >> 7);
    }
    const int p = (s + 4096) >> 13;
    return p < 0 ? 0 : (p > kBicubicPMax ? kBicubicPMax : p);
}

struct BicubicP { int p[4]; };
constexpr BicubicP bicubic_p(const uint32_t (&t)[16], int phiX, int phiY) {
    const BicubicRow wx = bicubic_row(phiX), wy = bicubic_row(phiY);
    return BicubicP{{bicubic_channel(t, 0, wx, wy), bicubic_channel(t, 1, wx, wy), bicubic_channel(t, 2, wx, wy),
                     bicubic_channel(t, 3, wx, wy)}};
}

// p as a sample value: ((float)p / 255.0f) * 2^-8, the division correctly rounded.  The two-operation form of
// lfg_device.hpp's unorm8_to_float (1 / 255 split in two floats, one fma) is that quotient for every p in [0, 65280], not only
// for the bytes: tests/cpp/bicubic_on_host.cpp goes through all 65,281, and an fma rounds the same on host and device.
#if defined(__HIP__)
#define LFG_BICUBIC_INLINE __host__ __device__ inline
#else
#define LFG_BICUBIC_INLINE inline
#endif
LFG_BICUBIC_INLINE float bicubic_p_to_float(int p) {
    const float k = (float)p, lo = k * -0x1.fdfdfep-33f;
    return __builtin_fmaf(k, 0x1.010102p-8f, lo) * 0.00390625f;
}

}  // namespace lfg
