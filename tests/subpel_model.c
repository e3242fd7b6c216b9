/* CPU model of lfg_motion_subpel and lfg_interpolate_compensated_subpel (include/linuxfg_hip.h): the fractional sample, the
 * two-stage search and its order; the fractional gate, the projection with its 64-bit key, the hole fill and the sampling, in
 * the header's operation order.  Built with the system C compiler and -ffp-contract=off by tests/subpel_model.py.  The
 * library's helpers, the bilinear fetch and the end of the sampling are tests/compensated_model.h's.
 *
 * Frames are tight: prev / curr / out RGBA8 rows of W * 4 bytes, mv int8 (x, y) pairs in rows of W * 2 bytes, mvq int16
 * (x, y) pairs in rows of W * 4 bytes, K 64-bit words in rows of W.
 *
 * Mutants, for the test of the tests alone (tests/test_subpel_model.py: the shared cases must tell each of them from the
 * model); with no such macro defined this file is the model:
 *   SUBPEL_MUTANT_SHORTEST_W   ties go to the smallest (|w|^2, wy, wx) instead of the smallest (|d|^2, dy, dx), d = w - 4v;
 *   SUBPEL_MUTANT_ROUND_SHIFT  the integer part of a vector as (w + 2) >> 2 instead of the floor w >> 2;
 *   SUBPEL_MUTANT_ROUND_7      the fractional sample rounded with + 7 instead of + 8;
 *   SUBPEL_MUTANT_STAGE2_AT_4V stage 2 centred on 4v instead of stage 1's winner h. */
#include "compensated_model.h"

#define QLIMIT 508
#define QHOLE 0xFFFFFFFFFFFFFFFFull

static inline int qclamp(int c) { return c < -QLIMIT ? -QLIMIT : (c > QLIMIT ? QLIMIT : c); }

/* prevq(r, w): four channels into p */
static void prevq(const uint8_t *prev, int W, int H, int rx, int ry, int wx, int wy, uint8_t *p) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
#ifdef SUBPEL_MUTANT_ROUND_SHIFT
    const int ix = rx + ((wx + 2) >> 2), iy = ry + ((wy + 2) >> 2);
#else
    const int ix = rx + (wx >> 2), iy = ry + (wy >> 2);
#endif
    const int fx = wx & 3, fy = wy & 3;
    const uint8_t *t[4];
    for (int k = 0; k < 4; ++k) {
        const int x = ix + (k & 1), y = iy + (k >> 1);
        t[k] = (x >= 0 && x < W && y >= 0 && y < H) ? prev + ((size_t)y * W + x) * 4 : zero;
    }
    for (int c = 0; c < 4; ++c) {
#ifdef SUBPEL_MUTANT_ROUND_7
        const int round = 7;
#else
        const int round = 8;
#endif
        p[c] = (uint8_t)(((4 - fx) * (4 - fy) * t[0][c] + fx * (4 - fy) * t[1][c] + (4 - fx) * fy * t[2][c] + fx * fy * t[3][c] + round) >> 4);
    }
}

static uint32_t cost_of(const uint8_t *prev, const uint8_t *curr, int W, int H, int qx, int qy, int wx, int wy, int R) {
    uint32_t cost = 0;
    for (int j = -R; j <= R; ++j)
        for (int i = -R; i <= R; ++i) {
            const int rx = qx + i, ry = qy + j;
            if (rx < 0 || rx >= W || ry < 0 || ry >= H) continue;
            uint8_t p[4];
            prevq(prev, W, H, rx, ry, wx, wy, p);
            cost += texel_sad(curr + ((size_t)ry * W + rx) * 4, p);
        }
    return cost;
}

/* is candidate (cost, w) before the best so far?  d = w - 4v */
static int before(uint32_t cost, int wx, int wy, int vx4, int vy4, uint32_t bcost, int bx, int by) {
    if (cost != bcost) return cost < bcost;
#ifdef SUBPEL_MUTANT_SHORTEST_W
    const int ax = wx, ay = wy, cx = bx, cy = by;
    (void)vx4; (void)vy4;
#else
    const int ax = wx - vx4, ay = wy - vy4, cx = bx - vx4, cy = by - vy4;
#endif
    const int la = ax * ax + ay * ay, lc = cx * cx + cy * cy;
    if (la != lc) return la < lc;
    if (ay != cy) return ay < cy;
    return ax < cx;
}

static void stage(const uint8_t *prev, const uint8_t *curr, int W, int H, int qx, int qy, int R, int vx4, int vy4, int cx, int cy,
                  int step, int *ox, int *oy) {
    int have = 0, bx = 0, by = 0;
    uint32_t bcost = 0;
    for (int b = -1; b <= 1; ++b)
        for (int a = -1; a <= 1; ++a) {
            const int wx = cx + a * step, wy = cy + b * step;
            if (wx < -QLIMIT || wx > QLIMIT || wy < -QLIMIT || wy > QLIMIT) continue;
            const uint32_t cost = cost_of(prev, curr, W, H, qx, qy, wx, wy, R);
            if (!have || before(cost, wx, wy, vx4, vy4, bcost, bx, by)) { have = 1; bcost = cost; bx = wx; by = wy; }
        }
    *ox = bx; *oy = by;
}

void subpel_refine(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, int W, int H, int R, int16_t *out) {
    for (int qy = 0; qy < H; ++qy)
        for (int qx = 0; qx < W; ++qx) {
            int vx = mv[((size_t)qy * W + qx) * 2], vy = mv[((size_t)qy * W + qx) * 2 + 1];
            if (vx < -127) vx = -127;
            if (vy < -127) vy = -127;
            int hx, hy, wx, wy;
            stage(prev, curr, W, H, qx, qy, R, 4 * vx, 4 * vy, 4 * vx, 4 * vy, 2, &hx, &hy);
#ifdef SUBPEL_MUTANT_STAGE2_AT_4V
            hx = 4 * vx; hy = 4 * vy;
#endif
            stage(prev, curr, W, H, qx, qy, R, 4 * vx, 4 * vy, hx, hy, 1, &wx, &wy);
            out[((size_t)qy * W + qx) * 2] = (int16_t)wx;
            out[((size_t)qy * W + qx) * 2 + 1] = (int16_t)wy;
        }
}

/* ---- the compensated route */

static int matched_q(const uint8_t *prev, const uint8_t *curr, const int16_t *mvq, int W, int H, int qx, int qy, int match_sad) {
    uint8_t p[4];
    prevq(prev, W, H, qx, qy, qclamp(mvq[((size_t)qy * W + qx) * 2]), qclamp(mvq[((size_t)qy * W + qx) * 2 + 1]), p);
    return texel_sad(curr + ((size_t)qy * W + qx) * 4, p) <= (uint32_t)match_sad;
}

/* the key of a projected vector: the smallest key is the longest vector, then the smallest wy, then the smallest wx */
static uint64_t qkey_of(int wx, int wy) {
    return ((uint64_t)(0xFFFFF - (wx * wx + wy * wy)) << 20) | ((uint64_t)(wy + 512) << 10) | (uint64_t)(wx + 512);
}

static void qdecode(uint64_t key, int *ux, int *uy) {
    *ux = (int)(key & 0x3FFu) - 512;
    *uy = (int)((key >> 10) & 0x3FFu) - 512;
}

static uint64_t qwalk_order(uint64_t key) { return ((0xFFFFFull - (key >> 20)) << 20) | (key & 0xFFFFFull); }

void subpel_project(const uint8_t *prev, const uint8_t *curr, const int16_t *mvq, int W, int H, float t, int match_sad, uint64_t *K) {
    const float s = 1.0f - t;
    for (size_t i = 0; i < (size_t)W * H; ++i) K[i] = QHOLE;
    for (int qy = 0; qy < H; ++qy)
        for (int qx = 0; qx < W; ++qx) {
            if (!matched_q(prev, curr, mvq, W, H, qx, qy, match_sad)) continue;
            const int wx = qclamp(mvq[((size_t)qy * W + qx) * 2]), wy = qclamp(mvq[((size_t)qy * W + qx) * 2 + 1]);
            const int dx = (int)floorf(((float)wx * 0.25f) * s + 0.5f), dy = (int)floorf(((float)wy * 0.25f) * s + 0.5f);
            const int x = qx + dx, y = qy + dy;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            if (qkey_of(wx, wy) < K[(size_t)y * W + x]) K[(size_t)y * W + x] = qkey_of(wx, wy);
        }
}

static void qfill_vector(const uint64_t *K, int W, int H, int x, int y, int *ux, int *uy) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
    uint64_t best = QHOLE;
    for (int k = 0; k < 4; ++k)
        for (int j = 1; j <= WALK; ++j) {
            const int nx = x + dir[k][0] * j, ny = y + dir[k][1] * j;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
            const uint64_t key = K[(size_t)ny * W + nx];
            if (key == QHOLE) continue;
            if (qwalk_order(key) < best) best = qwalk_order(key);
            break;
        }
    if (best == QHOLE) { *ux = 0; *uy = 0; return; }
    qdecode(best, ux, uy);
}

void subpel_sample(const uint8_t *prev, const uint8_t *curr, const int16_t *mvq, const uint64_t *K, int W, int H, float t,
                   int match_sad, int x0, int y0, int x1, int y1, uint8_t *out) {
    const float s = 1.0f - t;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            uint8_t *o = out + ((size_t)(y - y0) * (x1 - x0) + (x - x0)) * 4;
            const uint64_t key = K[(size_t)y * W + x];
            int ux, uy;
            const int hole = key == QHOLE;
            if (hole) qfill_vector(K, W, H, x, y, &ux, &uy);
            else qdecode(key, &ux, &uy);
            const float Px = ((float)x + 0.5f) + ((float)ux * 0.25f) * t, Py = ((float)y + 0.5f) + ((float)uy * 0.25f) * t;
            const float Cx = ((float)x + 0.5f) - ((float)ux * 0.25f) * s, Cy = ((float)y + 0.5f) - ((float)uy * 0.25f) * s;
            const vec4 Pv = bilinear_px(prev, W, H, Px, Py), Cv = bilinear_px(curr, W, H, Cx, Cy);
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                if (!matched_q(prev, curr, mvq, W, H, cx, cy, match_sad)) { store(o, Cv); continue; }     /* revealed */
                const int16_t *v = mvq + ((size_t)cy * W + cx) * 2;
                if (qclamp(v[0]) != ux || qclamp(v[1]) != uy) { store(o, Pv); continue; }                 /* covered */
            }
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}
