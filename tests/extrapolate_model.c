/* CPU model of lfg_extrapolate_compensated (include/linuxfg_hip.h): the match gate, the projection past time 1, the hole walk
 * with its donor rule and the sampling of curr, in the header's fp32 operation order.  Built with the system C compiler and
 * -ffp-contract=off by tests/extrapolate_model.py.  The library's helpers, the gate and the key are
 * tests/compensated_model.h's, shared with the family's other models; this file holds the projection, the walk that reports
 * its donor and the donor rule.
 *
 * Frames are tight: prev / curr / out RGBA8 rows of W * 4 bytes, mv int8 (x, y) pairs in rows of W * 2 bytes.
 *
 * ex_project: the key image K (W * H words) of one factor.  ex_sample: output pixels [x0, x1) x [y0, y1) from K, written to
 * out in rows of (x1 - x0) pixels; branch (same layout, one byte per pixel, or NULL) says how each pixel was made: 0 a projected
 * pixel, 1 a hole with no donor, 2 a hole with a donor whose C stayed, 3 a hole that took the donor branch.
 *
 * Mutants, for the test of the tests alone (tests/test_extrapolate_model.py: the shared cases must tell each of them from the
 * model); with no such macro defined this file is the model:
 *   EX_MUTANT_PLUS_V         the projection with +v instead of -v;
 *   EX_MUTANT_CEIL_PROJECT   the projection as ceilf(-v * a - 0.5) instead of floorf(0.5 - v * a);
 *   EX_MUTANT_ONE_MINUS_A    the sample offset taken with 1 - a instead of a;
 *   EX_MUTANT_NO_DONOR       the donor rule dropped: C always stays;
 *   EX_MUTANT_LATER_TIE      on an equal triple the later direction wins. */
#include "compensated_model.h"

void ex_project(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, int W, int H, float a, int match_sad, uint32_t *K) {
    for (size_t i = 0; i < (size_t)W * H; ++i) K[i] = HOLE;
    for (int qy = 0; qy < H; ++qy)
        for (int qx = 0; qx < W; ++qx) {
            if (!matched(prev, curr, mv, W, H, qx, qy, match_sad)) continue;
            const int vx = mv[((size_t)qy * W + qx) * 2], vy = mv[((size_t)qy * W + qx) * 2 + 1];
#if defined(EX_MUTANT_PLUS_V)
            const int dx = (int)floorf(0.5f + (float)vx * a), dy = (int)floorf(0.5f + (float)vy * a);
#elif defined(EX_MUTANT_CEIL_PROJECT)
            const int dx = (int)ceilf(-((float)vx * a) - 0.5f), dy = (int)ceilf(-((float)vy * a) - 0.5f);
#else
            const int dx = (int)floorf(0.5f - (float)vx * a), dy = (int)floorf(0.5f - (float)vy * a);
#endif
            const int x = qx + dx, y = qy + dy;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            if (key_of(vx, vy) < K[(size_t)y * W + x]) K[(size_t)y * W + x] = key_of(vx, vy);
        }
}

/* The donor of hole (x, y): of the first non-hole pixel in each of the directions +x, -x, +y, -y within WALK, the one with the
 * smallest (|v|^2, vy, vx), the earlier direction on an equal triple.  Returns 0, with u = (0, 0), if there is none. */
static int find_donor(const uint32_t *K, int W, int H, int x, int y, int *ux, int *uy, int *nx, int *ny) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
    uint32_t best = HOLE;
    for (int k = 0; k < 4; ++k)
        for (int j = 1; j <= WALK; ++j) {
            const int qx = x + dir[k][0] * j, qy = y + dir[k][1] * j;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) break;
            const uint32_t key = K[(size_t)qy * W + qx];
            if (key == HOLE) continue;
            const uint32_t order = walk_order(key);
#ifdef EX_MUTANT_LATER_TIE
            if (order <= best) { best = order; *nx = qx; *ny = qy; }
#else
            if (order < best) { best = order; *nx = qx; *ny = qy; }
#endif
            break;
        }
    if (best == HOLE) { *ux = 0; *uy = 0; return 0; }
    decode(best, ux, uy);
    return 1;
}

void ex_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint32_t *K, int W, int H, float a,
               int match_sad, int x0, int y0, int x1, int y1, uint8_t *out, uint8_t *branch) {
#ifdef EX_MUTANT_ONE_MINUS_A
    const float f = 1.0f - a;
#else
    const float f = a;
#endif
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const size_t o = (size_t)(y - y0) * (x1 - x0) + (x - x0);
            const uint32_t key = K[(size_t)y * W + x];
            int ux, uy, nx = x, ny = y, how = 0;
            if (key != HOLE) decode(key, &ux, &uy);
            else how = find_donor(K, W, H, x, y, &ux, &uy, &nx, &ny) ? 2 : 1;
            float Cx = ((float)x + 0.5f) + (float)ux * f, Cy = ((float)y + 0.5f) + (float)uy * f;
#ifndef EX_MUTANT_NO_DONOR
            if (how == 2) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                const int8_t *v = mv + ((size_t)cy * W + cx) * 2;
                if (matched(prev, curr, mv, W, H, cx, cy, match_sad) && (v[0] != ux || v[1] != uy)) {
                    Cx = ((float)nx + 0.5f) + (float)ux * f;     /* the foreground is at c: the background's edge, stretched */
                    Cy = ((float)ny + 0.5f) + (float)uy * f;
                    how = 3;
                }
            }
#endif
            store(out + o * 4, bilinear_px(curr, W, H, Cx, Cy));
            if (branch) branch[o] = (uint8_t)how;
        }
}
