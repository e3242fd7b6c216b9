/* What the CPU models of the compensated family share (mc_model.c, overlay_model.c, extrapolate_model.c, bidir_model.c): the
 * library's own helpers restated once, in the header's fp32 operation order, for a build with -ffp-contract=off.  On the kernel
 * side each of them has one home too: the hole word, the match gate, the hole walk (mc_fill_vector) and the end of a pixel
 * (mc_store_inside_or_blend) in linux-fg_amd/csrc/lfg_mc.hpp, the key, its decode and the flip to the walk's order in
 * lfg_vector_word.hpp, the taps and the UNORM8 conversions in lfg_interp.hpp.
 *
 * Only what means the same in every model lives here.  A step that differs between two models (a projection, a walk that
 * passes static pixels or reports its donor, a hole rule) is a function of that model's own file, with its mutant macros
 * around it: no macro and no flag selects behaviour in this file. */
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define HOLE 0xFFFFFFFFu
#define WALK 16

typedef struct { float x, y, z, w; } vec4;

/* UNORM8 -> float is (float)k / 255; the store clamps, scales by 255 and rounds half to even */
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

/* the gate of `own`'s pixel q against `far` at q + a(q), far outside the image read as 0 */
static inline int gate(const uint8_t *own, const uint8_t *far, const int8_t *a, int W, int H, int qx, int qy, int match_sad) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    const int sx = qx + a[((size_t)qy * W + qx) * 2], sy = qy + a[((size_t)qy * W + qx) * 2 + 1];
    const uint8_t *p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? far + ((size_t)sy * W + sx) * 4 : zero;
    return texel_sad(own + ((size_t)qy * W + qx) * 4, p) <= (uint32_t)match_sad;
}

/* the one-field gate: curr(q) against prev(q + mv(q)) */
static inline int matched(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, int W, int H, int qx, int qy, int match_sad) {
    return gate(curr, prev, mv, W, H, qx, qy, match_sad);
}

/* the key of a projected vector: the smallest key is the longest vector, then the smallest vy, then the smallest vx */
static inline uint32_t key_of(int vx, int vy) {
    return ((uint32_t)(65535 - (vx * vx + vy * vy)) << 16) | ((uint32_t)(vy + 128) << 8) | (uint32_t)(vx + 128);
}

/* ... whose low half gives the vector back */
static inline void decode(uint32_t key, int *ux, int *uy) {
    *ux = (int)(key & 0xffu) - 128;
    *uy = (int)((key >> 8) & 0xffu) - 128;
}

/* a stored key as the hole walk orders it, (|v|^2 << 16) | (vy + 128) << 8 | (vx + 128): the smallest is the shortest vector */
static inline uint32_t walk_order(uint32_t key) { return ((65535u - (key >> 16)) << 16) | (key & 0xffffu); }

/* texture() with CLAMP_TO_EDGE, in pixel units: (px, py) is a position with texel centres at i + 0.5 */
static inline vec4 bilinear_px(const uint8_t *img, int W, int H, float px, float py) {
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

/* The fill vector of hole (x, y): of the first non-hole pixel in each axis direction within WALK, the smallest
 * (|v|^2, vy, vx); (0, 0) if there is none. */
static inline void fill_vector(const uint32_t *K, int W, int H, int x, int y, int *ux, int *uy) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
    uint32_t best = HOLE;
    for (int k = 0; k < 4; ++k)
        for (int j = 1; j <= WALK; ++j) {
            const int nx = x + dir[k][0] * j, ny = y + dir[k][1] * j;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
            const uint32_t key = K[(size_t)ny * W + nx];
            if (key == HOLE) continue;
            if (walk_order(key) < best) best = walk_order(key);
            break;
        }
    if (best == HOLE) { *ux = 0; *uy = 0; return; }
    decode(best, ux, uy);
}

/* The end of an interpolated pixel that no rule has decided: the sample whose position alone is inside the image, else the
 * blend of prev's sample Pv at P and curr's Cv at C. */
static inline void store_inside_or_blend(uint8_t *o, vec4 Pv, vec4 Cv, float Px, float Py, float Cx, float Cy, int W, int H,
                                         float t) {
    const int pin = inside(Px, Py, W, H), cin = inside(Cx, Cy, W, H);
    if (pin && !cin) store(o, Pv);
    else if (cin && !pin) store(o, Cv);
    else {
        const vec4 m = {mixf(Pv.x, Cv.x, t), mixf(Pv.y, Cv.y, t), mixf(Pv.z, Cv.z, t), mixf(Pv.w, Cv.w, t)};
        store(o, m);
    }
}
