// Test helper (CPU only): holds csrc/lfg_vector_word.hpp -- the MV_S8X2 word, the order key of a vector, the compensated
// family's longest-first key -- to the expressions the kernels spelled out before they shared it, copied below verbatim, and
// both keys to the tuple orders they stand for.  Prints "ok <cases>" and exits 0, or prints the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

#include "lfg_vector_word.hpp"

namespace {

// ---- the kernels' own expressions, verbatim ----
// pack: motion_lean / motion_strip / motion_resolve / prefilter_epilogue (16-bit), motion_literal (32-bit), motion_pyramid
uint16_t old_pack16(int dx, int dy) { return (uint16_t)(uint8_t)(int8_t)(dx) | (uint16_t)((uint16_t)(uint8_t)(int8_t)(dy) << 8); }
uint32_t old_pack32(int dx, int dy) { return (uint32_t)(uint8_t)(int8_t)(dx) | ((uint32_t)(uint8_t)(int8_t)(dy) << 8); }
uint16_t old_pack_pyramid(int vx, int vy) { return (uint16_t)((uint32_t)(vx & 0xff) | ((uint32_t)(vy & 0xff) << 8)); }
// ... and motion_refine, from the low half of its key
uint16_t old_pack_refine(uint64_t best) { return (uint16_t)(((uint32_t)best ^ 0x8080u) & 0xffffu); }
// unpack: interpolate_mc (mv_at, a 16-bit word), pair_stats / motion_refine (the word in 32 bits), motion_pyramid
struct OldMv { int x, y; };
OldMv old_mv_at(uint16_t w) { return OldMv{(int)(int8_t)(w & 0xffu), (int)(int8_t)(w >> 8)}; }
OldMv old_unpack32(uint32_t vec) { return OldMv{(int)(int8_t)(vec & 0xffu), (int)(int8_t)(vec >> 8)}; }
OldMv old_unpack_pyramid(uint16_t pv) { return OldMv{(int)(int8_t)(pv & 0xffu), (int)(int8_t)(pv >> 8)}; }
// the order key: motion_pyramid (cand_rank), motion_refine (below its cost)
uint32_t old_cand_rank(int vx, int vy) { return ((uint32_t)(vx * vx + vy * vy) << 16) | ((uint32_t)(vy + 128) << 8) | (uint32_t)(vx + 128); }
uint64_t old_refine_key(uint32_t cost, int vx, int vy) {
    return ((uint64_t)cost << 32) | ((uint64_t)(vx * vx + vy * vy) << 16) | ((uint64_t)(vy + 128) << 8) | (uint64_t)(vx + 128);
}
// its decode: motion_pyramid (store_quad), interpolate_mc (mc_decode)
OldMv old_decode(uint32_t r) { return OldMv{(int)(r & 0xffu) - 128, (int)((r >> 8) & 0xffu) - 128}; }
// interpolate_mc: the longest-first key, and the hole walk's way back to the order key
uint32_t old_mc_key(int x, int y) { return ((uint32_t)(65535 - (x * x + y * y)) << 16) | ((uint32_t)(y + 128) << 8) | (uint32_t)(x + 128); }
uint32_t old_hole_order(uint32_t n) { return ((65535u - (n >> 16)) << 16) | (n & 0xffffu); }

long long cases = 0;
bool fail(const char *what, long long a, long long b) {
    std::printf("%s differs at (%lld, %lld)\n", what, a, b);
    return false;
}
#define HOLD(cond, what, a, b) do { ++cases; if (!(cond)) return fail(what, (long long)(a), (long long)(b)); } while (0)

bool check() {
    using namespace lfg;
    // every word: unpack then pack gives it back, and unpack is each former spelling
    for (uint32_t w = 0; w < 65536u; ++w) {
        const Mv v = mv_unpack((uint16_t)w);
        HOLD(mv_word(v.x, v.y) == w, "pack(unpack(word))", w, 0);
        HOLD(v.x >= -128 && v.x <= 127 && v.y >= -128 && v.y <= 127, "unpack's range", w, 0);
        const OldMv a = old_mv_at((uint16_t)w), b = old_unpack32(w), c = old_unpack_pyramid((uint16_t)w);
        HOLD(v.x == a.x && v.y == a.y && v.x == b.x && v.y == b.y && v.x == c.x && v.y == c.y, "unpack", w, 0);
    }
    // pack: every spelling, also where a component leaves the S8 range and wraps (+128 is stored as -128)
    for (int dy = -130; dy <= 130; ++dy)
        for (int dx = -130; dx <= 130; ++dx) {
            HOLD(mv_word(dx, dy) == old_pack16(dx, dy), "pack (16-bit spelling)", dx, dy);
            HOLD((uint32_t)mv_word(dx, dy) == old_pack32(dx, dy), "pack (32-bit spelling)", dx, dy);
            HOLD(mv_word(dx, dy) == old_pack_pyramid(dx, dy), "pack (pyramid's spelling)", dx, dy);
        }
    // the keys, for every vector an MV_S8X2 word can hold
    for (int vy = -128; vy <= 127; ++vy)
        for (int vx = -128; vx <= 127; ++vx) {
            const uint32_t key = mv_order_key(vx, vy);
            HOLD(key == old_cand_rank(vx, vy), "order key", vx, vy);
            for (uint32_t cost : {0u, 1u, 0xFFFFFFFFu})
                HOLD((((uint64_t)cost << 32) | key) == old_refine_key(cost, vx, vy), "cost above the order key", vx, vy);
            const Mv d = mv_order_decode(key);
            const OldMv od = old_decode(key);
            HOLD(d.x == vx && d.y == vy && od.x == vx && od.y == vy, "order key's decode", vx, vy);
            HOLD(mv_word(d.x, d.y) == old_pack_refine(((uint64_t)7 << 32) | key), "word of a key", vx, vy);
            const uint32_t lf = mv_longest_first_key(vx, vy);
            HOLD(lf == old_mc_key(vx, vy), "longest-first key", vx, vy);
            HOLD(mv_key_flip_length(lf) == key && old_hole_order(lf) == key, "longest-first key back to the order key", vx, vy);
            const Mv ld = mv_order_decode(lf);
            HOLD(ld.x == vx && ld.y == vy, "longest-first key's decode", vx, vy);
        }
    for (uint32_t hi = 0; hi < 65536u; ++hi)
        for (uint32_t lo : {0u, 0x8080u, 0xFFFFu}) {
            const uint32_t n = (hi << 16) | lo;
            HOLD(mv_key_flip_length(n) == old_hole_order(n) && mv_key_flip_length(mv_key_flip_length(n)) == n, "length flip", hi, lo);
        }
    // Both keys against the tuple orders they stand for, on all pairs.  Components run to the ends of what the word holds, -128
    // and 127: +128 has no S8 value, and a key's byte fields cannot hold 128 + 128 either.
    const int comp[] = {-128, -127, -100, -64, -33, -17, -16, -9, -8, -3, -2, -1, 0, 1, 2, 3, 8, 9, 16, 17, 33, 64, 100, 126, 127};
    std::vector<Mv> vs;
    for (int y : comp)
        for (int x : comp) vs.push_back(Mv{x, y});
    for (const Mv &a : vs)
        for (const Mv &b : vs) {
            const int la = a.x * a.x + a.y * a.y, lb = b.x * b.x + b.y * b.y;
            HOLD((mv_order_key(a.x, a.y) < mv_order_key(b.x, b.y)) == (std::make_tuple(la, a.y, a.x) < std::make_tuple(lb, b.y, b.x)),
                 "order key against (|v|^2, vy, vx)", mv_word(a.x, a.y), mv_word(b.x, b.y));
            HOLD((mv_longest_first_key(a.x, a.y) < mv_longest_first_key(b.x, b.y)) == (std::make_tuple(-la, a.y, a.x) < std::make_tuple(-lb, b.y, b.x)),
                 "longest-first key against (-|v|^2, vy, vx)", mv_word(a.x, a.y), mv_word(b.x, b.y));
        }
    return true;
}

// (the header's functions are constexpr: a few of the above at compile time as well)
static_assert(lfg::mv_word(-1, 2) == 0x02FFu && lfg::mv_unpack(0x02FFu).x == -1 && lfg::mv_unpack(0x02FFu).y == 2, "MV_S8X2");
static_assert(lfg::mv_order_key(0, 0) == ((128u << 8) | 128u), "the zero vector's key");

}  // namespace

int main() {
    if (!check()) return 1;
    std::printf("ok %lld\n", cases);
    return 0;
}
