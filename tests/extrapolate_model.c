/* CPU model of lfg_extrapolate_compensated (include/linuxfg_hip.h): the match gate, the projection past time 1, the hole walk
 * with its donor rule and the sampling of curr, in the header's fp32 operation order.  Built with the system C compiler and
 * -ffp-contract=off by tests/extrapolate_model.py.
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
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define HOLE 0xFFFFFFFFu
#define WALK 16

typedef struct { float x, y, z, w; } vec4;

/* the library's own helpers, restated: UNORM8 -> float is (float)k / 255, the store clamps, scales by 255 and rounds half
 * to even */
static inline float unorm(uint8_t b) { return (float)b / 255.0f; }

static inline uint8_t pack_unorm(float v) {
    float x = v * 255.0f;
    if (!(x > 0.0f)) x = 0.0f;
    if (x > 255.0f) x = 255.0f;
    return (uint8_t)lrintf(x);
}

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static inline uint32_t texel_sad(const uint8_t *a, const uint8_t *b) {
    uint32_t s = 0;
    for (int c = 0; c < 4; ++c) s += (uint32_t)abs((int)a[c] - (int)b[c]);
    return s;
}

/* the gate: curr(q) against prev(q + mv(q)), prev outside the image read as 0 */
static int matched(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, int W, int H, int qx, int qy, int match_sad) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    const int8_t *v = mv + ((size_t)qy * W + qx) * 2;
    const int sx = qx + v[0], sy = qy + v[1];
    const uint8_t *p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? prev + ((size_t)sy * W + sx) * 4 : zero;
    return texel_sad(curr + ((size_t)qy * W + qx) * 4, p) <= (uint32_t)match_sad;
}

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
            const uint32_t key = ((uint32_t)(65535 - (vx * vx + vy * vy)) << 16) | ((uint32_t)(vy + 128) << 8) | (uint32_t)(vx + 128);
            if (key < K[(size_t)y * W + x]) K[(size_t)y * W + x] = key;
        }
}

/* texture() with CLAMP_TO_EDGE, in pixel units: (px, py) is a position with texel centres at i + 0.5 */
static vec4 bilinear_px(const uint8_t *img, int W, int H, float px, float py) {
    const float u = px - 0.5f, v = py - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float a = u - fu, b = v - fv;
    const int i0 = clampi((int)fu, 0, W - 1), i1 = clampi((int)fu + 1, 0, W - 1);
    const int j0 = clampi((int)fv, 0, H - 1), j1 = clampi((int)fv + 1, 0, H - 1);
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    const uint8_t *t00 = img + ((size_t)j0 * W + i0) * 4, *t10 = img + ((size_t)j0 * W + i1) * 4;
    const uint8_t *t01 = img + ((size_t)j1 * W + i0) * 4, *t11 = img + ((size_t)j1 * W + i1) * 4;
    float r[4];
    for (int c = 0; c < 4; ++c)
        r[c] = ((w00 * unorm(t00[c]) + w10 * unorm(t10[c])) + w01 * unorm(t01[c])) + w11 * unorm(t11[c]);
    vec4 o = {r[0], r[1], r[2], r[3]};
    return o;
}

static inline void store(uint8_t *o, vec4 v) {
    o[0] = pack_unorm(v.x); o[1] = pack_unorm(v.y); o[2] = pack_unorm(v.z); o[3] = pack_unorm(v.w);
}

static inline void decode(uint32_t key, int *ux, int *uy) {
    *ux = (int)(key & 0xffu) - 128;
    *uy = (int)((key >> 8) & 0xffu) - 128;
}

/* The donor of hole (x, y): of the first non-hole pixel in each of the directions +x, -x, +y, -y within WALK, the one with the
 * smallest (|v|^2, vy, vx), the earlier direction on an equal triple.  Returns 0, with u = (0, 0), if there is none. */
static int find_donor(const uint32_t *K, int W, int H, int x, int y, int *ux, int *uy, int *nx, int *ny) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
    uint32_t best = HOLE;                                      /* (|v|^2 << 16) | (vy + 128) << 8 | (vx + 128) */
    for (int k = 0; k < 4; ++k)
        for (int j = 1; j <= WALK; ++j) {
            const int qx = x + dir[k][0] * j, qy = y + dir[k][1] * j;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) break;
            const uint32_t key = K[(size_t)qy * W + qx];
            if (key == HOLE) continue;
            const uint32_t order = ((65535u - (key >> 16)) << 16) | (key & 0xffffu);
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
