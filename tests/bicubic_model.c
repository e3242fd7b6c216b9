/* CPU model of the bicubic fetch and of lfg_interpolate_compensated_sampled with LFG_SAMPLING_BICUBIC (include/linuxfg_hip.h):
 * the table from the rational rule in integers, the fetch as the header writes it, and the sampling step of both routes with
 * it.  Built with the system C compiler and -ffp-contract=off by tests/bicubic_model.py.  The library's helpers, the gate, the
 * key, the plain hole walk and the end of the sampling are tests/compensated_model.h's; the sub-pixel route's gate, key and walk
 * are tests/subpel_model.c's own functions, taken by including that file as it is (its entry points come along unused).  The
 * projections are not restated: tests/mc_model.py and tests/subpel_model.py make the key images.
 *
 * Frames are tight, as in those two models.
 *
 * Mutants, for the test of the tests alone (tests/test_bicubic_model.py: named cases must tell each of them from the model);
 * with no such macro defined this file is the model:
 *   BICUBIC_MUTANT_TRUNC_SHIFT  h_r as (sum + 64) / 128, truncated toward zero, instead of the floor >> 7;
 *   BICUBIC_MUTANT_ROUND_PHASE  the phase rounded to nearest, (int)(a * 64 + 0.5), instead of truncated;
 *   BICUBIC_MUTANT_NO_CLAMP     p not clamped to [0, 65280].
 * And one rewrite that is no mutant, kept so that the test can say so: BICUBIC_MUTANT_WRONG_TAP puts the remainder of 16384 on
 * tap 2 for phi <= 32 and on tap 1 above; the remainder is zero at every phase, so the table is the same. */
#include "subpel_model.c"

/* Wt[phi][0..3] for any phi in [0, 64] */
static void weights_of(int phi, int w[4]) {
    const int64_t f = phi, n[4] = {-4096 * f + 128 * f * f - f * f * f, 524288 - 320 * f * f + 3 * f * f * f,
                                   4096 * f + 256 * f * f - 3 * f * f * f, -64 * f * f + f * f * f};
    for (int k = 0; k < 4; ++k) {
        const int64_t v = n[k] + 16;
        w[k] = (int)(v >= 0 ? v / 32 : -((-v + 31) / 32));                 /* the floor, without relying on >> of a negative */
    }
#ifdef BICUBIC_MUTANT_WRONG_TAP
    const int rest = phi <= 32 ? 2 : 1;
#else
    const int rest = phi <= 32 ? 1 : 2;
#endif
    w[rest] = 0;
    w[rest] = 16384 - (w[0] + w[1] + w[2] + w[3]);
}

void bicubic_table(int16_t *out) {
    for (int phi = 0; phi < 64; ++phi) {
        int w[4];
        weights_of(phi, w);
        for (int k = 0; k < 4; ++k) out[4 * phi + k] = (int16_t)w[k];
    }
}

static int floor_div(int v, int d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }

/* the integer body at texel (i, j) and phases (phix, phiy): p[4]; ext, if given, collects min / max of h_r and of s */
void bicubic_body(const uint8_t *img, int W, int H, int i, int j, int phix, int phiy, int32_t *p, int32_t *ext) {
    int wx[4], wy[4];
    weights_of(phix, wx);
    weights_of(phiy, wy);
    for (int c = 0; c < 4; ++c) {
        int s = 0;
        for (int r = 0; r < 4; ++r) {
            const int y = clampi(j - 1 + r, 0, H - 1);
            int sum = 0;
            for (int k = 0; k < 4; ++k) sum += wx[k] * img[((size_t)y * W + clampi(i - 1 + k, 0, W - 1)) * 4 + c];
#ifdef BICUBIC_MUTANT_TRUNC_SHIFT
            const int h = (sum + 64) / 128;
#else
            const int h = floor_div(sum + 64, 128);
#endif
            if (ext) { if (h < ext[0]) ext[0] = h; if (h > ext[1]) ext[1] = h; }
            s += wy[r] * h;
        }
        if (ext) { if (s < ext[2]) ext[2] = s; if (s > ext[3]) ext[3] = s; }
        int v = floor_div(s + 4096, 8192);
#ifndef BICUBIC_MUTANT_NO_CLAMP
        v = v < 0 ? 0 : (v > 65280 ? 65280 : v);
#endif
        p[c] = v;
    }
}

/* the phases of position (px, py): for the tests' coverage count */
void bicubic_phases(float px, float py, int32_t *phases) {
    const float u = px - 0.5f, v = py - 0.5f;
    const float a = u - floorf(u), b = v - floorf(v);
#ifdef BICUBIC_MUTANT_ROUND_PHASE
    phases[0] = (int)(a * 64.0f + 0.5f); phases[1] = (int)(b * 64.0f + 0.5f);
#else
    phases[0] = (int)(a * 64.0f); phases[1] = (int)(b * 64.0f);
#endif
}

static vec4 bicubic_px(const uint8_t *img, int W, int H, float px, float py) {
    const float u = px - 0.5f, v = py - 0.5f;
    int32_t ph[2], p[4];
    bicubic_phases(px, py, ph);
    bicubic_body(img, W, H, (int)floorf(u), (int)floorf(v), ph[0], ph[1], p, 0);
    const vec4 o = {((float)p[0] / 255.0f) * 0.00390625f, ((float)p[1] / 255.0f) * 0.00390625f,
                    ((float)p[2] / 255.0f) * 0.00390625f, ((float)p[3] / 255.0f) * 0.00390625f};
    return o;
}

/* one fetch as floats, for tests of the fetch alone */
void bicubic_fetch(const uint8_t *img, int W, int H, float px, float py, float *out) {
    const vec4 v = bicubic_px(img, W, H, px, py);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
}

/* mc_model.c's mc_sample with the bicubic fetch; `phases`, if given, counts the phases of every fetch: 65 x, then 65 y */
void bicubic_mc_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint32_t *K, int W, int H, float t,
                       int match_sad, int x0, int y0, int x1, int y1, uint8_t *out, uint32_t *phases) {
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
            if (phases) {
                int32_t ph[2];
                bicubic_phases(Px, Py, ph); phases[ph[0]]++; phases[65 + ph[1]]++;
                bicubic_phases(Cx, Cy, ph); phases[ph[0]]++; phases[65 + ph[1]]++;
            }
            const vec4 Pv = bicubic_px(prev, W, H, Px, Py), Cv = bicubic_px(curr, W, H, Cx, Cy);
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                if (!matched(prev, curr, mv, W, H, cx, cy, match_sad)) { store(o, Cv); continue; }     /* revealed */
                const int8_t *v = mv + ((size_t)cy * W + cx) * 2;
                if (v[0] != ux || v[1] != uy) { store(o, Pv); continue; }                              /* covered */
            }
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}

/* subpel_model.c's subpel_sample with the bicubic fetch */
void bicubic_subpel_sample(const uint8_t *prev, const uint8_t *curr, const int16_t *mvq, const uint64_t *K, int W, int H, float t,
                           int match_sad, int x0, int y0, int x1, int y1, uint8_t *out, uint32_t *phases) {
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
            if (phases) {
                int32_t ph[2];
                bicubic_phases(Px, Py, ph); phases[ph[0]]++; phases[65 + ph[1]]++;
                bicubic_phases(Cx, Cy, ph); phases[ph[0]]++; phases[65 + ph[1]]++;
            }
            const vec4 Pv = bicubic_px(prev, W, H, Px, Py), Cv = bicubic_px(curr, W, H, Cx, Cy);
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                if (!matched_q(prev, curr, mvq, W, H, cx, cy, match_sad)) { store(o, Cv); continue; }     /* revealed */
                const int16_t *v = mvq + ((size_t)cy * W + cx) * 2;
                if (qclamp(v[0]) != ux || qclamp(v[1]) != uy) { store(o, Pv); continue; }                 /* covered */
            }
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}
