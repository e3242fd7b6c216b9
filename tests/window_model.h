/* What the CPU models of the window-cost family share (refine_model.c, expand_model.c): the cost of an integer vector and the
 * key whose minimum wins, restated once from include/linuxfg_hip.h in integer arithmetic.  On the kernel side both have one
 * home too, linux-fg_amd/csrc/lfg_window_cost.hpp, with the key's low half and its decode in lfg_vector_word.hpp.
 *
 * Only what means the same in every model lives here: no macro and no flag selects behaviour in this file.  A departure
 * (expand_model.c's TIE_VX_FIRST key) is a function of that model's own file, under its mutant macro.  subpel_model.c's
 * cost_of samples prev fractionally and pyramid_model.c's cost is another rule: both stay on their own. */
#pragma once
#include <stdint.h>
#include <stdlib.h>

/* (cost, |v|^2, vy, vx), most significant first */
static inline uint64_t key_of(uint32_t cost, int vx, int vy) {
    return ((uint64_t)cost << 32) | ((uint64_t)(vx * vx + vy * vy) << 16) | ((uint64_t)(vy + 128) << 8) | (uint64_t)(vx + 128);
}

static inline int key_vx(uint64_t key) { return (int)(key & 0xff) - 128; }
static inline int key_vy(uint64_t key) { return (int)((key >> 8) & 0xff) - 128; }

/* sum over the window texels r inside the image of sum_c |curr(r)_c - prev(r + v)_c|, prev outside the image read as 0 */
static uint32_t cost_at(const uint8_t *prev, const uint8_t *curr, int W, int H, int qx, int qy, int vx, int vy, int radius) {
    uint32_t s = 0;
    for (int ry = qy - radius; ry <= qy + radius; ++ry)
        for (int rx = qx - radius; rx <= qx + radius; ++rx) {
            if (rx < 0 || rx >= W || ry < 0 || ry >= H) continue;
            const uint8_t *c = curr + ((size_t)ry * W + rx) * 4;
            const int sx = rx + vx, sy = ry + vy;
            const int in = sx >= 0 && sx < W && sy >= 0 && sy < H;
            for (int ch = 0; ch < 4; ++ch) {
                const int p = in ? prev[((size_t)sy * W + sx) * 4 + ch] : 0;
                s += (uint32_t)abs((int)c[ch] - p);
            }
        }
    return s;
}
