/* CPU model of lfg_frame_halve and lfg_motion_expand (include/linuxfg_hip.h): the rounded 2 x 2 mean, the doubled 3 x 3
 * coarse neighbours, the +-1 parity step, with the window cost and the key order of window_model.h, in integer arithmetic
 * exactly as the header defines them.  Built with the system C compiler by tests/expand_model.py.
 *
 * Frames are tight: prev / curr RGBA8 rows of W * 4 bytes, mv_low int8 (x, y) pairs in rows of ceil(W / 2) * 2 bytes.
 *
 * expand_roi: output vectors of the pixels [x0, x1) x [y0, y1), written to out in rows of (x1 - x0) pixels.
 *
 * -DEXPAND_MUTANT_<name> builds one deliberate departure from the definition (tests/test_expand_model.py tells each from the
 * model by a named case of tests/expand_cases.py):
 *   NO_SATURATION   doubling wraps in the byte instead of saturating at +-127
 *   NO_PARITY       step 2 omitted: the output is the coarse neighbour w
 *   NEIGHBOURS_2X2  the neighbours (a, b) in {0, 1}^2 instead of {-1, 0, 1}^2
 *   ROUND_UP        the centre neighbour at ((x + 1) >> 1, (y + 1) >> 1)
 *   TIE_VX_FIRST    the key (cost, |v|^2, vx, vy) */
#include "window_model.h"

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

void expand_halve(const uint8_t *in, int W, int H, uint8_t *out) {
    const int Wd = (W + 1) / 2, Hd = (H + 1) / 2;
    for (int y = 0; y < Hd; ++y)
        for (int x = 0; x < Wd; ++x)
            for (int c = 0; c < 4; ++c) {
                int sum = 2;
                for (int j = 0; j < 2; ++j)
                    for (int i = 0; i < 2; ++i)
                        sum += in[((size_t)clampi(2 * y + j, 0, H - 1) * W + clampi(2 * x + i, 0, W - 1)) * 4 + c];
                out[((size_t)y * Wd + x) * 4 + c] = (uint8_t)(sum >> 2);
            }
}

/* this model's key: window_model.h's, or TIE_VX_FIRST's (cost, |v|^2, vx, vy), which is that key of the transposed vector */
static inline uint64_t expand_key(uint32_t cost, int vx, int vy) {
#ifdef EXPAND_MUTANT_TIE_VX_FIRST
    return key_of(cost, vy, vx);
#else
    return key_of(cost, vx, vy);
#endif
}

static inline int dbl(int v) {
#ifdef EXPAND_MUTANT_NO_SATURATION
    return (int8_t)(uint8_t)(2 * v);
#else
    return clampi(2 * v, -127, 127);
#endif
}

void expand_roi(const uint8_t *prev, const uint8_t *curr, const int8_t *mv_low, int W, int H, int radius,
                int x0, int y0, int x1, int y1, int8_t *out) {
    const int Wl = (W + 1) / 2, Hl = (H + 1) / 2;
    for (int qy = y0; qy < y1; ++qy)
        for (int qx = x0; qx < x1; ++qx) {
#ifdef EXPAND_MUTANT_ROUND_UP
            const int cx = clampi((qx + 1) >> 1, 0, Wl - 1), cy = clampi((qy + 1) >> 1, 0, Hl - 1);
#else
            const int cx = qx >> 1, cy = qy >> 1;
#endif
#ifdef EXPAND_MUTANT_NEIGHBOURS_2X2
            const int first = 0;
#else
            const int first = -1;
#endif
            /* step 1: the coarse neighbour */
            uint64_t best = ~(uint64_t)0;
            for (int b = first; b <= 1; ++b)
                for (int a = first; a <= 1; ++a) {
                    const int nx = cx + a, ny = cy + b;
                    if (nx < 0 || nx >= Wl || ny < 0 || ny >= Hl) continue;
                    const int vx = dbl(mv_low[((size_t)ny * Wl + nx) * 2]), vy = dbl(mv_low[((size_t)ny * Wl + nx) * 2 + 1]);
                    const uint64_t key = expand_key(cost_at(prev, curr, W, H, qx, qy, vx, vy, radius), vx, vy);
                    if (key < best) best = key;
                }
#ifdef EXPAND_MUTANT_TIE_VX_FIRST
            const int wx = key_vy(best), wy = key_vx(best);
#else
            const int wx = key_vx(best), wy = key_vy(best);
#endif
            int ox = wx, oy = wy;
#ifndef EXPAND_MUTANT_NO_PARITY
            /* step 2: the parity */
            best = ~(uint64_t)0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int vx = clampi(wx + dx, -127, 127), vy = clampi(wy + dy, -127, 127);
                    const uint64_t key = expand_key(cost_at(prev, curr, W, H, qx, qy, vx, vy, radius), vx, vy);
                    if (key < best) { best = key; ox = vx; oy = vy; }
                }
#endif
            int8_t *o = out + ((size_t)(qy - y0) * (x1 - x0) + (qx - x0)) * 2;
            o[0] = (int8_t)ox;
            o[1] = (int8_t)oy;
        }
}
