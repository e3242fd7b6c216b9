// The MV_S8X2 word of a motion vector and the total orders the opt-in stages put on vectors.  Host and device code
// share this header; it needs nothing but the standard library, so that tests/cpp/vector_word_check.cpp can hold
// every definition to the expression it replaces with g++ alone.  In use: mv_word at every store of a vector, and every
// unpack, key and decode of the opt-in stages (the pyramid, the compensated family through lfg_mc.hpp, motion_refine.hip,
// pair_stats.hip).  What the default path's kernels still spell themselves is listed in DESIGN.md section 4.10.
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

}  // namespace lfg
