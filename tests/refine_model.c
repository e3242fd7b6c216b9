/* CPU model of lfg_motion_refine (include/linuxfg_hip.h): the 17 candidates, with the window cost and the key order of
 * window_model.h, in integer arithmetic exactly as the header defines them.  Built with the system C compiler by
 * tests/refine_model.py.
 *
 * Frames are tight: prev / curr RGBA8 rows of W * 4 bytes, mv int8 (x, y) pairs in rows of W * 2 bytes.
 *
 * refine_roi: output vectors of the pixels [x0, x1) x [y0, y1), written to out in rows of (x1 - x0) pixels. */
#include "window_model.h"

static const int DX[17] = {0, -4, 0, 4, -4, 4, -4, 0, 4, -8, 0, 8, -8, 8, -8, 0, 8};
static const int DY[17] = {0, -4, -4, -4, 0, 0, 4, 4, 4, -8, -8, -8, 0, 0, 8, 8, 8};

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
            o[0] = (int8_t)key_vx(best);
            o[1] = (int8_t)key_vy(best);
        }
}
