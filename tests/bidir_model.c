/* CPU model of lfg_interpolate_compensated_bidirectional and lfg_motion_consistency (include/linuxfg_hip.h): the two
 * `confirmed` predicates, both projections, the hole fill, the symmetric hole rule and the sampling, in the header's fp32
 * operation order.  Built with the system C compiler and -ffp-contract=off by tests/bidir_model.py.
 *
 * Frames are tight: prev / curr / out RGBA8 rows of W * 4 bytes, fwd / bwd int8 (x, y) pairs in rows of W * 2 bytes, masks rows
 * of W bytes.
 *
 * bidir_consistency: the vector half of the predicates.  bidir_project: the key image K (W * H words) of one factor.
 * bidir_sample: output pixels [x0, x1) x [y0, y1) from K, written to out in rows of (x1 - x0) pixels.
 *
 * Mutants, for the test of the tests alone (tests/test_bidir_model.py: a case must tell each of them from the model); with no
 * such macro defined this file is the model:
 *   BIDIR_MUTANT_NEG128_AS_127  a backward vector with a component of -128 is not refused: the component is carried as 127;
 *   BIDIR_MUTANT_CHEBYSHEV      the tolerance bounds max(|dx|, |dy|) instead of |dx| + |dy|;
 *   BIDIR_MUTANT_STRICT         `<` for `<=` in the tolerance. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define HOLE 0xFFFFFFFFu
#define WALK 16

typedef struct { float x, y, z, w; } vec4;

/* the library's own helpers, restated as tests/mc_model.c restates them */
static inline float unorm(uint8_t b) { return (float)b / 255.0f; }

static inline uint8_t pack_unorm(float v) {
    float x = v * 255.0f;
    if (!(x > 0.0f)) x = 0.0f;
    if (x > 255.0f) x = 255.0f;
    return (uint8_t)lrintf(x);
}

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static inline float mixf(float x, float y, float a) { return x * (1.0f - a) + y * a; }

static inline uint32_t texel_sad(const uint8_t *a, const uint8_t *b) {
    uint32_t s = 0;
    for (int c = 0; c < 4; ++c) s += (uint32_t)abs((int)a[c] - (int)b[c]);
    return s;
}

static inline uint32_t key_of(int vx, int vy) {
    return ((uint32_t)(65535 - (vx * vx + vy * vy)) << 16) | ((uint32_t)(vy + 128) << 8) | (uint32_t)(vx + 128);
}

/* r = q + a(q) inside the image and the other field there within the tolerance of -a(q) */
static int consistent(const int8_t *a, const int8_t *b, int W, int H, int qx, int qy, int tolerance) {
    const int ax = a[((size_t)qy * W + qx) * 2], ay = a[((size_t)qy * W + qx) * 2 + 1];
    const int rx = qx + ax, ry = qy + ay;
    if (rx < 0 || rx >= W || ry < 0 || ry >= H) return 0;
    const int ex = abs(ax + b[((size_t)ry * W + rx) * 2]), ey = abs(ay + b[((size_t)ry * W + rx) * 2 + 1]);
#if defined(BIDIR_MUTANT_CHEBYSHEV)
    return (ex > ey ? ex : ey) <= tolerance;
#elif defined(BIDIR_MUTANT_STRICT)
    return ex + ey < tolerance;
#else
    return ex + ey <= tolerance;
#endif
}

/* the gate of `own`'s pixel q against `far` at q + a(q), far outside the image read as 0 */
static int gate(const uint8_t *own, const uint8_t *far, const int8_t *a, int W, int H, int qx, int qy, int match_sad) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    const int sx = qx + a[((size_t)qy * W + qx) * 2], sy = qy + a[((size_t)qy * W + qx) * 2 + 1];
    const uint8_t *p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? far + ((size_t)sy * W + sx) * 4 : zero;
    return texel_sad(own + ((size_t)qy * W + qx) * 4, p) <= (uint32_t)match_sad;
}

static int confirmed_f(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, int W, int H, int qx, int qy,
                       int match_sad, int tolerance) {
    return gate(curr, prev, fwd, W, H, qx, qy, match_sad) && consistent(fwd, bwd, W, H, qx, qy, tolerance);
}

static int confirmed_b(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, int W, int H, int px, int py,
                       int match_sad, int tolerance) {
#ifndef BIDIR_MUTANT_NEG128_AS_127
    if (bwd[((size_t)py * W + px) * 2] == -128 || bwd[((size_t)py * W + px) * 2 + 1] == -128) return 0;
#endif
    return gate(prev, curr, bwd, W, H, px, py, match_sad) && consistent(bwd, fwd, W, H, px, py, tolerance);
}

/* the vector that the content of prev's pixel carries in fwd's convention: -b */
static inline int carried(int b) {
#ifdef BIDIR_MUTANT_NEG128_AS_127
    if (b == -128) return 127;
#endif
    return -b;
}

void bidir_consistency(const int8_t *a, const int8_t *b, int W, int H, int tolerance, uint8_t *out) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) out[(size_t)y * W + x] = consistent(a, b, W, H, x, y, tolerance) ? 255 : 0;
}

static void put(uint32_t *K, int W, int H, int x, int y, uint32_t key) {
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    if (key < K[(size_t)y * W + x]) K[(size_t)y * W + x] = key;
}

/* which = 1: the forward projection alone, 2: the backward one alone, 3: both (the call's K) */
void bidir_project(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, int W, int H, float t,
                   int match_sad, int tolerance, int which, uint32_t *K) {
    const float s = 1.0f - t;
    for (size_t i = 0; i < (size_t)W * H; ++i) K[i] = HOLE;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            if ((which & 1) && confirmed_f(prev, curr, fwd, bwd, W, H, x, y, match_sad, tolerance)) {
                const int fx = fwd[((size_t)y * W + x) * 2], fy = fwd[((size_t)y * W + x) * 2 + 1];
                put(K, W, H, x + (int)floorf((float)fx * s + 0.5f), y + (int)floorf((float)fy * s + 0.5f), key_of(fx, fy));
            }
            if ((which & 2) && confirmed_b(prev, curr, fwd, bwd, W, H, x, y, match_sad, tolerance)) {
                const int bx = bwd[((size_t)y * W + x) * 2], by = bwd[((size_t)y * W + x) * 2 + 1];
                put(K, W, H, x + (int)floorf((float)bx * t + 0.5f), y + (int)floorf((float)by * t + 0.5f), key_of(carried(bx), carried(by)));
            }
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

static inline int inside(float x, float y, int W, int H) { return x >= 0.0f && x <= (float)W && y >= 0.0f && y <= (float)H; }

static inline void store(uint8_t *o, vec4 v) {
    o[0] = pack_unorm(v.x); o[1] = pack_unorm(v.y); o[2] = pack_unorm(v.z); o[3] = pack_unorm(v.w);
}

static inline void decode(uint32_t key, int *ux, int *uy) {
    *ux = (int)(key & 0xffu) - 128;
    *uy = (int)((key >> 8) & 0xffu) - 128;
}

/* The fill vector of hole (x, y): of the first non-hole pixel in each axis direction within WALK, the smallest
 * (|v|^2, vy, vx); (0, 0) if there is none. */
static void fill_vector(const uint32_t *K, int W, int H, int x, int y, int *ux, int *uy) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
    uint32_t best = HOLE;                                      /* (|v|^2 << 16) | (vy + 128) << 8 | (vx + 128) */
    for (int k = 0; k < 4; ++k)
        for (int j = 1; j <= WALK; ++j) {
            const int nx = x + dir[k][0] * j, ny = y + dir[k][1] * j;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
            const uint32_t key = K[(size_t)ny * W + nx];
            if (key == HOLE) continue;
            const uint32_t order = ((65535u - (key >> 16)) << 16) | (key & 0xffffu);
            if (order < best) best = order;
            break;
        }
    if (best == HOLE) { *ux = 0; *uy = 0; return; }
    decode(best, ux, uy);
}

void bidir_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, const uint32_t *K, int W, int H,
                  float t, int match_sad, int tolerance, int x0, int y0, int x1, int y1, uint8_t *out) {
    const float s = 1.0f - t;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            uint8_t *o = out + ((size_t)(y - y0) * (x1 - x0) + (x - x0)) * 4;
            const uint32_t key = K[(size_t)y * W + x];
            int ux, uy;
            const int hole = key == HOLE;
            if (hole) fill_vector(K, W, H, x, y, &ux, &uy);
            else decode(key, &ux, &uy);
            const float Px = ((float)x + 0.5f) + (float)ux * t, Py = ((float)y + 0.5f) + (float)uy * t;
            const float Cx = ((float)x + 0.5f) - (float)ux * s, Cy = ((float)y + 0.5f) - (float)uy * s;
            const vec4 Pv = bilinear_px(prev, W, H, Px, Py), Cv = bilinear_px(curr, W, H, Cx, Cy);
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                const int px = clampi((int)floorf(Px), 0, W - 1), py = clampi((int)floorf(Py), 0, H - 1);
                const int8_t *f = fwd + ((size_t)cy * W + cx) * 2, *b = bwd + ((size_t)py * W + px) * 2;
                const int cbad = confirmed_f(prev, curr, fwd, bwd, W, H, cx, cy, match_sad, tolerance) && (f[0] != ux || f[1] != uy);
                const int pbad = confirmed_b(prev, curr, fwd, bwd, W, H, px, py, match_sad, tolerance) &&
                                 (carried(b[0]) != ux || carried(b[1]) != uy);
                if (cbad && !pbad) { store(o, Pv); continue; }                                        /* covered in curr */
                if (pbad && !cbad) { store(o, Cv); continue; }                                        /* revealed in curr */
            }
            const int pin = inside(Px, Py, W, H), cin = inside(Cx, Cy, W, H);
            if (pin && !cin) store(o, Pv);
            else if (cin && !pin) store(o, Cv);
            else {
                const vec4 m = {mixf(Pv.x, Cv.x, t), mixf(Pv.y, Cv.y, t), mixf(Pv.z, Cv.z, t), mixf(Pv.w, Cv.w, t)};
                store(o, m);
            }
        }
}
