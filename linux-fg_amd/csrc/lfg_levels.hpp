// Level matching in integers (lfg_frame_histogram, lfg_levels_match, lfg_levels_apply, include/linuxfg_hip.h; DESIGN.md
// section 4.26): the rule that turns two histogram records into a pair of monotone level maps, the gate that decides whether
// the pair is levelled at all, and the two point-wise bodies that apply a map to a texel.  Host and device code share this
// header; it needs nothing but the standard library, so that the kernels (levels.hip) and tests/cpp/levels_on_host.cpp, built
// with g++ alone, run the same text.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LFG_LEVELS_FN __host__ __device__ inline
#else
#define LFG_LEVELS_FN inline
#endif

namespace lfg {

constexpr int kLevels = 256;                   // levels of a channel
constexpr int kLevelChannels = 3;              // channels that have a map: alpha has none
constexpr int kLevelsMaxShift16 = 4080;        // 255 levels in sixteenths

// The words of the two records (include/linuxfg_hip.h): a histogram record is pixels, then hist[4][256]; a map is pixels,
// shift_sum, (active, reserved), then forward[3][256] and inverse[3][256] as bytes.
constexpr int kHistWords = 1 + 4 * kLevels;
constexpr int kMapHeadBytes = 24;
constexpr int kMapBytes = kMapHeadBytes + 2 * kLevelChannels * kLevels;

// cdf[v] = hist[0] + .. + hist[v], in 64 bits.
LFG_LEVELS_FN void levels_cdf(const uint64_t *hist, uint64_t *cdf) {
    uint64_t sum = 0;
    for (int v = 0; v < kLevels; ++v) { sum += hist[v]; cdf[v] = sum; }
}

// The smallest w with cdf[w] >= target; 255 where there is none (records of unequal counts, which the gate leaves alone).
// cdf is non-decreasing, so eight halvings find it.
LFG_LEVELS_FN uint32_t levels_rank(const uint64_t *cdf, uint64_t target) {
    uint32_t lo = 0, hi = kLevels - 1;             // the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] >= target) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One level's share of shift_sum: hist * |mapped - v|.
LFG_LEVELS_FN uint64_t levels_shift(uint64_t hist, uint32_t mapped, uint32_t v) {
    return hist * (uint64_t)(mapped > v ? mapped - v : v - mapped);
}

// The gate, in 64 bits as the header writes it.
LFG_LEVELS_FN bool levels_active(uint64_t pixelsFrom, uint64_t pixelsTo, uint64_t shiftSum, int minShift16) {
    return pixelsFrom == pixelsTo && pixelsFrom != 0 && 16u * shiftSum >= (uint64_t)minShift16 * 3u * pixelsFrom;
}

// LFG_LEVELS_AT's weight of the frame itself: t in 256ths, rounded to nearest.
LFG_LEVELS_FN int levels_tq(float factor) { return (int)floorf(factor * 256.0f + 0.5f); }

// One level through LFG_LEVELS_AT: the level itself at tq = 256, its inverse at tq = 0.
LFG_LEVELS_FN uint32_t levels_at(uint32_t inverse, uint32_t v, int tq) {
    return ((uint32_t)(256 - tq) * inverse + (uint32_t)tq * v + 128u) >> 8;
}

// A texel through a table of three rows of 256 bytes (forward, or levels_at of inverse): alpha is kept.
LFG_LEVELS_FN uint32_t levels_texel(const uint8_t *table, uint32_t p) {
    return (uint32_t)table[p & 0xffu] | ((uint32_t)table[kLevels + ((p >> 8) & 0xffu)] << 8) |
           ((uint32_t)table[2 * kLevels + ((p >> 16) & 0xffu)] << 16) | (p & 0xff000000u);
}

// The whole rule on the host, as the match kernel runs it in parallel: `from` and `to` are records of kHistWords words, `map`
// kMapBytes bytes.  tests/cpp/levels_on_host.cpp calls this; the kernel calls the pieces above.
inline void levels_match_host(const uint64_t *from, const uint64_t *to, int minShift16, uint8_t *map) {
    uint64_t cdfFrom[kLevelChannels][kLevels], cdfTo[kLevelChannels][kLevels];
    uint8_t *forward = map + kMapHeadBytes, *inverse = forward + kLevelChannels * kLevels;
    uint64_t shiftSum = 0;
    for (int c = 0; c < kLevelChannels; ++c) {
        levels_cdf(from + 1 + c * kLevels, cdfFrom[c]);
        levels_cdf(to + 1 + c * kLevels, cdfTo[c]);
        for (int v = 0; v < kLevels; ++v) {
            const uint32_t f = levels_rank(cdfTo[c], cdfFrom[c][v]);
            forward[c * kLevels + v] = (uint8_t)f;
            inverse[c * kLevels + v] = (uint8_t)levels_rank(cdfFrom[c], cdfTo[c][v]);
            shiftSum += levels_shift(from[1 + c * kLevels + v], f, (uint32_t)v);
        }
    }
    const bool active = levels_active(from[0], to[0], shiftSum, minShift16);
    if (!active)
        for (int i = 0; i < kLevelChannels * kLevels; ++i) forward[i] = inverse[i] = (uint8_t)(i % kLevels);
    uint64_t head[3] = {from[0], shiftSum, active ? 1u : 0u};     // (active, reserved) as one little-endian word
    for (int i = 0; i < kMapHeadBytes; ++i) map[i] = (uint8_t)(head[i / 8] >> (8 * (i % 8)));
}

}  // namespace lfg
