// The MV_S8X2 word of a motion vector and the total orders the opt-in stages put on vectors.  Host and device code
// share this header; it needs nothing but the standard library, so that tests/cpp/vector_word_check.cpp can hold
// every definition to the expression it replaces with g++ alone.  In use: mv_word at every store of a vector, and every
// unpack, key and decode of the opt-in stages (the pyramid, the compensated family through lfg_mc.hpp, motion_refine.hip,
// pair_stats.hip).  What the default path's kernels still spell themselves is listed in DESIGN.md section 4.10.  Below them the
// MV_S16X2_Q2 word of a quarter-pixel vector and its keys (motion_subpel.hip, interpolate_subpel.hip).
#pragma once

#include <cstdint>

namespace lfg {

struct Mv { int x, y; };
// LFG_FORMAT_MV_S8X2: dx in the low byte, dy in the high one, both two's complement.
constexpr uint16_t mv_word(int dx, int dy) {
    return (uint16_t)((uint16_t)(uint8_t)(int8_t)dx | (uint16_t)((uint16_t)(uint8_t)(int8_t)dy << 8));
}
constexpr Mv mv_unpack(uint16_t word) { return Mv{(int)(int8_t)(word & 0xffu), (int)(int8_t)(word >> 8)}; }
// The order key: the smallest key is the smallest (|v|^2, vy, vx).  Components in [-128, 127]: |v|^2 <= 32768 fits the high half.
constexpr uint32_t mv_order_key(int vx, int vy) {
    return ((uint32_t)(vx * vx + vy * vy) << 16) | ((uint32_t)(vy + 128) << 8) | (uint32_t)(vx + 128);
}
// ... whose low half alone gives the vector back (a key may carry a cost above bit 31: only the low 16 bits are decoded).
constexpr Mv mv_order_decode(uint32_t key) { return Mv{(int)(key & 0xffu) - 128, (int)((key >> 8) & 0xffu) - 128}; }
// The same key with the length inverted, 65535 - |v|^2 in the high half, and back again: one function both ways.
constexpr uint32_t mv_key_flip_length(uint32_t key) { return ((65535u - (key >> 16)) << 16) | (key & 0xffffu); }
// The compensated family's key: the longest vector first, then the smallest vy, then the smallest vx.  It equals
// mv_key_flip_length(mv_order_key(vx, vy)) (tests/cpp/vector_word_check.cpp); spelled out because that composition costs each
// project kernel one more instruction.
constexpr uint32_t mv_longest_first_key(int vx, int vy) {
    return ((uint32_t)(65535 - (vx * vx + vy * vy)) << 16) | ((uint32_t)(vy + 128) << 8) | (uint32_t)(vx + 128);
}


// LFG_FORMAT_MV_S16X2_Q2: x in the low half, y in the high one, both two's complement, in quarter pixels.  A frame may hold
// any 16-bit values; every reader clamps each component to [-kMvqLimit, kMvqLimit] = 4 * [-127, 127], which mvq_unpack does.
constexpr int kMvqLimit = 508;
constexpr uint32_t mvq_word(int wx, int wy) {
    return (uint32_t)(uint16_t)(int16_t)wx | ((uint32_t)(uint16_t)(int16_t)wy << 16);
}
constexpr int mvq_clamp(int c) { return c < -kMvqLimit ? -kMvqLimit : (c > kMvqLimit ? kMvqLimit : c); }
constexpr Mv mvq_unpack(uint32_t word) {
    return Mv{mvq_clamp((int)(int16_t)(word & 0xffffu)), mvq_clamp((int)(int16_t)(word >> 16))};
}
// lfg_motion_subpel's order among candidates of one cost: the smallest (dx^2 + dy^2, dy, dx) of d = w - 4v, components in
// [-3, 3]; the low six bits alone give d back.
constexpr uint32_t mvq_delta_key(int dx, int dy) {
    return ((uint32_t)(dx * dx + dy * dy) << 6) | ((uint32_t)(dy + 3) << 3) | (uint32_t)(dx + 3);
}
constexpr Mv mvq_delta_decode(uint32_t key) { return Mv{(int)(key & 7u) - 3, (int)((key >> 3) & 7u) - 3}; }
// The order key of a clamped quarter-pixel vector, the smallest key the smallest (|w|^2, wy, wx): |w|^2 <= 2 * 508^2 needs 20
// bits and each component, offset by 512, 10.  The low 20 bits alone give the vector back.
constexpr uint64_t mvq_order_key(int wx, int wy) {
    return ((uint64_t)(uint32_t)(wx * wx + wy * wy) << 20) | ((uint64_t)(uint32_t)(wy + 512) << 10) | (uint64_t)(uint32_t)(wx + 512);
}
constexpr Mv mvq_order_decode(uint64_t key) { return Mv{(int)(key & 0x3ffu) - 512, (int)((key >> 10) & 0x3ffu) - 512}; }
// The same key with the length inverted, 0xFFFFF - |w|^2, and back again: one function both ways.
constexpr uint64_t mvq_key_flip_length(uint64_t key) { return ((0xfffffull - (key >> 20)) << 20) | (key & 0xfffffull); }
// The sub-pixel compensated route's key: the longest vector first, then the smallest wy, then the smallest wx.  Below 2^40,
// so the all-ones word is above every key.
constexpr uint64_t mvq_longest_first_key(int wx, int wy) {
    return ((uint64_t)(uint32_t)(0xfffff - (wx * wx + wy * wy)) << 20) | ((uint64_t)(uint32_t)(wy + 512) << 10) | (uint64_t)(uint32_t)(wx + 512);
}

}  // namespace lfg
