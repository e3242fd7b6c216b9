// Debanding with dithered output in integers (lfg_deband, include/linuxfg_hip.h): the random source, the
// draw of a pixel -- its tap offsets and its noise -- and what the pixel does with its taps once they are loaded: accept or
// refuse each iteration's average, add the noise, round.  Host and device code share this header; it needs nothing but the
// standard library, so that the kernel (deband.hip), lfg_deband_draw (lfg_capi.cpp) and tests/cpp/deband_on_host.cpp, built
// with g++ alone, run the same text.
//
// Ranges (iterations <= 4, threshold <= 64, radius <= 32, grain <= 16): S = radius * i <= 128 and 2 S + 1 <= 257, so the two
// offset products are 16 bits x 9 bits; a noise product is 8 bits x (4 + 2 grain <= 36): all of them fit the 24-bit multiply.
// v and s are at most 1020, v + n lies in [-16, 1039]: 16-bit halves carry the tap sums of two channels side by side.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define LFG_DEBAND_FN __host__ __device__ inline
#else
#define LFG_DEBAND_FN inline
#endif

namespace lfg {

constexpr int kDebandMaxIterations = 4, kDebandMaxThreshold = 64, kDebandMaxRadius = 32, kDebandMaxGrain = 16;
constexpr int kDebandTaps = 4;                              // taps of one iteration: the offset and its three quarter turns

// a * b for factors that fit 24 bits (the header's ranges).  Masked, which changes no value and tells the compiler, which does
// not know the range of a kernel argument: it takes the full-rate 24-bit multiply (lfg_resample.hpp: resample_mul24).
LFG_DEBAND_FN uint32_t deband_mul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }

// h(k): 32-bit arithmetic throughout.
LFG_DEBAND_FN uint32_t deband_hash(uint32_t k) {
    k ^= k >> 16; k *= 0x7feb352du;
    k ^= k >> 15; k *= 0x846ca68bu;
    k ^= k >> 16;
    return k;
}

// r0 = h(x ^ h(y ^ h(seed))) in three steps, the first the same for a whole call and the second for a whole row.
LFG_DEBAND_FN uint32_t deband_seed_key(uint32_t seed) { return deband_hash(seed); }
LFG_DEBAND_FN uint32_t deband_row_key(uint32_t seedKey, uint32_t y) { return deband_hash(y ^ seedKey); }
LFG_DEBAND_FN uint32_t deband_r0(uint32_t rowKey, uint32_t x) { return deband_hash(x ^ rowKey); }
// r_j = h(r0 + j): j = 1 .. 4 the iterations' offsets, j = 5 the noise.
LFG_DEBAND_FN uint32_t deband_r(uint32_t r0, uint32_t j) { return deband_hash(r0 + j); }
constexpr uint32_t kDebandNoiseDraw = 5u;

// (ox, oy) of r_i in the square [-S, S]^2, S = radius * i.
struct DebandOffset { int x, y; };

LFG_DEBAND_FN DebandOffset deband_offset(uint32_t r, int S) {
    const uint32_t span = 2u * (uint32_t)S + 1u;
    return DebandOffset{(int)(deband_mul24(r & 0xffffu, span) >> 16) - S, (int)(deband_mul24(r >> 16, span) >> 16) - S};
}

// Tap t = 0 .. 3 of an offset, relative to the pixel: (ox, oy), (-ox, -oy), (-oy, ox), (oy, -ox).
LFG_DEBAND_FN DebandOffset deband_tap(DebandOffset o, int t) {
    return t == 0 ? o : t == 1 ? DebandOffset{-o.x, -o.y} : t == 2 ? DebandOffset{-o.y, o.x} : DebandOffset{o.y, -o.x};
}

// p + d clamped to [0, n - 1]; p < n <= 2^30 (a row of n RGBA8 pixels has a 32-bit pitch) and |d| <= 128.
// (min(max(t, 0), last) is the form the compiler turns into one v_med3_i32.)
LFG_DEBAND_FN uint32_t deband_clamped(uint32_t p, int d, uint32_t n) {
    const int t = (int)p + d, last = (int)n - 1, m = t > 0 ? t : 0;
    return (uint32_t)(m < last ? m : last);
}

// n_c = ((b_c (4 + 2 G)) >> 8) - G for byte b_c of the noise draw.
LFG_DEBAND_FN int deband_noise(uint32_t b, int grain) { return (int)(deband_mul24(b, 4u + 2u * (uint32_t)grain) >> 8) - grain; }

// A value that has passed through here is not part of the shift-clamp-pack pattern that the compiler folds into an instruction
// the device gets wrong (yuv_convert.hip: kept_apart; the build's check_store_hazard.py refuses the instruction).
LFG_DEBAND_FN int deband_kept_apart(int v) {
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// One channel after its iterations: the noise, the rounding shift (arithmetic: floor) and the byte range.
LFG_DEBAND_FN uint32_t deband_round(int v, int n) {
    const int b = (v + n) >> 2;
    return (uint32_t)deband_kept_apart(b < 0 ? 0 : (b > 255 ? 255 : b));
}

// The pixel from its loaded texels: `c` the pixel itself, taps[4 (i - 1) + t] tap t of iteration i, all packed RGBA8 and all of
// `in`; `noise` is r_5.  Channels 0 .. 2: v = 4 c, replaced by an iteration's tap sum s where |s - v| <= threshold / i; then
// the noise and the rounding.  Channel 3 is c's.  The tap sums of channels 0 and 2 ride in one word and that of channel 1 in
// another (16-bit halves, <= 1020 each).  No branch: a refused iteration costs what an accepted one does.
template <int I>
LFG_DEBAND_FN uint32_t deband_texel(uint32_t c, const uint32_t (&taps)[kDebandTaps * I], int threshold, int grain, uint32_t noise) {
    int v[3] = {(int)(4u * (c & 255u)), (int)(4u * ((c >> 8) & 255u)), (int)(4u * ((c >> 16) & 255u))};
#pragma unroll
    for (int i = 0; i < I; ++i) {
        uint32_t even = 0u, odd = 0u;                       // channels 0 and 2; channels 1 and 3
#pragma unroll
        for (int t = 0; t < kDebandTaps; ++t) {
            even += taps[kDebandTaps * i + t] & 0x00ff00ffu;
            odd += (taps[kDebandTaps * i + t] >> 8) & 0x00ff00ffu;
        }
        const int s[3] = {(int)(even & 0xffffu), (int)(odd & 0xffffu), (int)(even >> 16)};
        const int limit = threshold / (i + 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int d = s[k] - v[k];
            v[k] = (d < 0 ? -d : d) <= limit ? s[k] : v[k];
        }
    }
    uint32_t px = c & 0xff000000u;
#pragma unroll
    for (int k = 0; k < 3; ++k) px |= deband_round(v[k], deband_noise((noise >> (8 * k)) & 255u, grain)) << (8 * k);
    return px;
}

}  // namespace lfg
