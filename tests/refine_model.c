/* CPU model of lfg_motion_refine (include/linuxfg_hip.h): the 17 candidates, the window cost and the key order, in integer
 * arithmetic exactly as the header defines them.  Built with the system C compiler by tests/refine_model.py.
 *
 * Frames are tight: prev / curr RGBA8 rows of W * 4 bytes, mv int8 (x, y) pairs in rows of W * 2 bytes.
 *
 * refine_roi: output vectors of the pixels [x0, x1) x [y0, y1), written to out in rows of (x1 - x0) pixels. */
#include <stdint.h>
#include <stdlib.h>

static const int DX[17] = {0, -4, 0, 4, -4, 4, -4, 0, 4, -8, 0, 8, -8, 8, -8, 0, 8};
static const int DY[17] = {0, -4, -4, -4, 0, 0, 4, 4, 4, -8, -8, -8, 0, 0, 8, 8, 8};

static inline uint64_t key_of(uint32_t cost, int vx, int vy) {
    return ((uint64_t)cost << 32) | ((uint64_t)(vx * vx + vy * vy) << 16) | ((uint64_t)(vy + 128) << 8) | (uint64_t)(vx + 128);
}

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

void refine_roi(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, int W, int H, int radius,
                int x0, int y0, int x1, int y1, int8_t *out) {
    for (int qy = y0; qy < y1; ++qy)
        for (int qx = x0; qx < x1; ++qx) {
            uint64_t best = ~(uint64_t)0;
            for (int k = 0; k < 17; ++k) {
                const int nx = qx + DX[k], ny = qy + DY[k];
                if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
                const int vx = mv[((size_t)ny * W + nx) * 2], vy = mv[((size_t)ny * W + nx) * 2 + 1];
                const uint64_t key = key_of(cost_at(prev, curr, W, H, qx, qy, vx, vy, radius), vx, vy);
                if (key < best) best = key;
            }
            int8_t *o = out + ((size_t)(qy - y0) * (x1 - x0) + (qx - x0)) * 2;
            o[0] = (int8_t)((int)(best & 0xff) - 128);
            o[1] = (int8_t)((int)((best >> 8) & 0xff) - 128);
        }
}
