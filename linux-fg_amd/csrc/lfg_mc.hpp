// What the compensated family shares (interpolate_mc.hip, extrapolate_mc.hip): the key image K's hole word, the packed-texel
// read, the vector read, the match gate, and the start of every launcher.  The vector word, the longest-first key that K
// holds (mv_longest_first_key), its decode (mv_order_decode) and the hole walks' way back to the order key
// (mv_key_flip_length) are lfg_vector_word.hpp's.
#pragma once

#include "lfg_device.hpp"
#include "lfg_internal.hpp"
#include "lfg_vector_word.hpp"

namespace lfg {

constexpr uint32_t kMcHole = 0xFFFFFFFFu;      // K where nothing was projected: what the clear leaves, above every key
constexpr int kMcBlockX = 64, kMcBlockY = 4;   // a wave is 64 pixels of one row

__device__ __forceinline__ uint32_t texel_u32(const uint8_t *__restrict__ img, size_t pitch, int x, int y) {
    return *reinterpret_cast<const uint32_t *>(img + (size_t)y * pitch + (size_t)x * 4u);
}

__device__ __forceinline__ Mv mv_at(const uint8_t *__restrict__ mv, size_t pitch, int x, int y) {
    return mv_unpack(*reinterpret_cast<const uint16_t *>(mv + (size_t)y * pitch + (size_t)x * 2u));
}

// The match gate: sum over the channels of |curr(q) - prev(q + v)| <= matchSad, prev outside the image read as 0.
// (pair_stats.hip counts the same comparison, on texels it has loaded a trip ahead.)
__device__ __forceinline__ bool matched(const uint8_t *__restrict__ prev, size_t prevPitch, uint32_t currTexel,
                                        int W, int H, int qx, int qy, Mv v, int matchSad) {
    const int sx = qx + v.x, sy = qy + v.y;
    const uint32_t p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? texel_u32(prev, prevPitch, sx, sy) : 0u;
    return __builtin_amdgcn_sad_u8(currTexel, p, 0u) <= (uint32_t)matchSad;
}

// Every launcher's start: K (W * H words) set to the hole word in stream order, and the grid of both launches, one thread
// per pixel in blocks of kMcBlockX x kMcBlockY.
inline dim3 mc_block() { return dim3(kMcBlockX, kMcBlockY); }
inline hipError_t mc_clear_keys(hipStream_t s, uint32_t *keys, int W, int H, dim3 &grid) {
    grid = dim3((unsigned)((W + kMcBlockX - 1) / kMcBlockX), (unsigned)((H + kMcBlockY - 1) / kMcBlockY));
    return hipMemsetAsync(keys, 0xFF, (size_t)W * (size_t)H * 4u, s);
}

}  // namespace lfg
