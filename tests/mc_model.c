/* CPU model of lfg_interpolate_compensated (include/linuxfg_hip.h): the match gate, the projection, the hole fill and the
 * sampling, in the header's fp32 operation order.  Built with the system C compiler and -ffp-contract=off by
 * tests/mc_model.py.  The library's helpers, the gate, the key, the plain hole walk and the end of the sampling are
 * tests/compensated_model.h's, shared with the family's other models; this file holds the projection and the hole rule.
 *
 * Frames are tight: prev / curr / out RGBA8 rows of W * 4 bytes, mv int8 (x, y) pairs in rows of W * 2 bytes.
 *
 * mc_project: the key image K (W * H words) of one factor.  mc_sample: output pixels [x0, x1) x [y0, y1) from K, written to
 * out in rows of (x1 - x0) pixels.
 *
 * Mutants, for the test of the tests alone (tests/test_mc_model.py: a set of factors must tell each of them from the model);
 * with no such macro defined this file is the model:
 *   MC_MUTANT_C_FROM_P      the curr sample position as C = P - u instead of C = (x + 0.5) - u * s;
 *   MC_MUTANT_CEIL_PROJECT  the projection as v - ceil(v * t - 0.5) instead of floor(v * s + 0.5);
 *   MC_MUTANT_HALF_LAST     the curr sample position as C = (x - u * s) + 0.5: the half pixel added last.
 * All are exact rewrites in real arithmetic and at every factor where the fp32 products are exact. */
#include "compensated_model.h"

void mc_project(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, int W, int H, float t, int match_sad, uint32_t *K) {
    const float s = 1.0f - t;
    for (size_t i = 0; i < (size_t)W * H; ++i) K[i] = HOLE;
    for (int qy = 0; qy < H; ++qy)
        for (int qx = 0; qx < W; ++qx) {
            if (!matched(prev, curr, mv, W, H, qx, qy, match_sad)) continue;
            const int vx = mv[((size_t)qy * W + qx) * 2], vy = mv[((size_t)qy * W + qx) * 2 + 1];
#ifdef MC_MUTANT_CEIL_PROJECT
            const int dx = vx - (int)ceilf((float)vx * t - 0.5f), dy = vy - (int)ceilf((float)vy * t - 0.5f);
            (void)s;
#else
            const int dx = (int)floorf((float)vx * s + 0.5f), dy = (int)floorf((float)vy * s + 0.5f);
#endif
            const int x = qx + dx, y = qy + dy;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            if (key_of(vx, vy) < K[(size_t)y * W + x]) K[(size_t)y * W + x] = key_of(vx, vy);
        }
}

void mc_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint32_t *K, int W, int H, float t,
               int match_sad, int x0, int y0, int x1, int y1, uint8_t *out) {
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
#if defined(MC_MUTANT_C_FROM_P)
            const float Cx = Px - (float)ux, Cy = Py - (float)uy;
            (void)s;
#elif defined(MC_MUTANT_HALF_LAST)
            const float Cx = ((float)x - (float)ux * s) + 0.5f, Cy = ((float)y - (float)uy * s) + 0.5f;
#else
            const float Cx = ((float)x + 0.5f) - (float)ux * s, Cy = ((float)y + 0.5f) - (float)uy * s;
#endif
            const vec4 Pv = bilinear_px(prev, W, H, Px, Py), Cv = bilinear_px(curr, W, H, Cx, Cy);
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                if (!matched(prev, curr, mv, W, H, cx, cy, match_sad)) { store(o, Cv); continue; }     /* revealed */
                const int8_t *v = mv + ((size_t)cy * W + cx) * 2;
                if (v[0] != ux || v[1] != uy) { store(o, Pv); continue; }                              /* covered */
            }
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}
