/* CPU model of lfg_interpolate_compensated_bidirectional and lfg_motion_consistency (include/linuxfg_hip.h): the two
 * `confirmed` predicates, both projections, the hole fill, the symmetric hole rule and the sampling, in the header's fp32
 * operation order.  Built with the system C compiler and -ffp-contract=off by tests/bidir_model.py.  The library's helpers,
 * the gate, the key, the hole walk and the end of the sampling are tests/compensated_model.h's, shared with the family's
 * other models; this file holds the predicates, the two projections and the symmetric hole rule.
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
#include "compensated_model.h"

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
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}
