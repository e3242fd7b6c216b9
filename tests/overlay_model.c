/* CPU model of lfg_interpolate_compensated_masked (include/linuxfg_hip.h): lfg_interpolate_compensated with a static mask,
 * in the header's fp32 operation order.  Built with the system C compiler and -ffp-contract=off by tests/overlay_model.py.
 * The library's helpers, the gate, the key and the end of the sampling are tests/compensated_model.h's, shared with the
 * family's other models; this file holds the projection with its static key, the walk that passes static pixels, the fetch
 * rule and the hole rule.  With an all-zero mask every step below is mc_model.c's (tests/test_overlay_model.py holds the two
 * to each other byte for byte).
 *
 * Frames are tight: prev / curr / out RGBA8 rows of W * 4 bytes, mv int8 (x, y) pairs in rows of W * 2 bytes, mask rows of W
 * bytes; a non-zero byte means static.
 *
 * ov_project: the key image K (W * H words) of one factor; a static location holds 0.  ov_sample: output pixels
 * [x0, x1) x [y0, y1) from K, written to out in rows of (x1 - x0) pixels.
 *
 * Mutants, for the test of the tests alone (tests/test_overlay_model.py: the shared cases must tell each of them from the
 * model); with no such macro defined this file is the model:
 *   OV_MUTANT_NO_PROJECT       a static pixel does not project its own vector (the stricter variant of DESIGN.md 4.13);
 *   OV_MUTANT_WALK_STOPS       the hole walk ends a direction at a static pixel, keeping nothing, instead of passing it;
 *   OV_MUTANT_RULE_AFTER_HOLE  the fetch rule tested after the hole's revealed / covered test instead of before it;
 *   OV_MUTANT_RULE_LRINT       the fetch rule's p and c from lrintf instead of floorf;
 *   OV_MUTANT_STATIC_CURR      a static location's output as curr(d) instead of mix(prev(d), curr(d), t). */
#include "compensated_model.h"

#define STATIC 0u

void ov_project(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint8_t *mask, int W, int H, float t,
                int match_sad, uint32_t *K) {
    const float s = 1.0f - t;
    for (size_t i = 0; i < (size_t)W * H; ++i) K[i] = HOLE;
    for (int qy = 0; qy < H; ++qy)
        for (int qx = 0; qx < W; ++qx) {
            if (mask[(size_t)qy * W + qx]) {
                K[(size_t)qy * W + qx] = STATIC;                /* the smallest key: whatever lands here, 0 stays */
#ifdef OV_MUTANT_NO_PROJECT
                continue;
#endif
            }
            if (!matched(prev, curr, mv, W, H, qx, qy, match_sad)) continue;
            const int vx = mv[((size_t)qy * W + qx) * 2], vy = mv[((size_t)qy * W + qx) * 2 + 1];
            const int dx = (int)floorf((float)vx * s + 0.5f), dy = (int)floorf((float)vy * s + 0.5f);
            const int x = qx + dx, y = qy + dy;
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            if (key_of(vx, vy) < K[(size_t)y * W + x]) K[(size_t)y * W + x] = key_of(vx, vy);
        }
}

/* The fill vector of hole (x, y): of the first pixel that is neither a hole nor static in each axis direction within WALK,
 * the smallest (|v|^2, vy, vx); (0, 0) if there is none.  An overlay is not the surface behind it, so this is not the
 * shared header's fill_vector, which knows no static pixel. */
static void fill_vector_past_static(const uint32_t *K, int W, int H, int x, int y, int *ux, int *uy) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
    uint32_t best = HOLE;
    for (int k = 0; k < 4; ++k)
        for (int j = 1; j <= WALK; ++j) {
            const int nx = x + dir[k][0] * j, ny = y + dir[k][1] * j;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
            const uint32_t key = K[(size_t)ny * W + nx];
            if (key == HOLE) continue;
#ifdef OV_MUTANT_WALK_STOPS
            if (key == STATIC) break;
#else
            if (key == STATIC) continue;
#endif
            if (walk_order(key) < best) best = walk_order(key);
            break;
        }
    if (best == HOLE) { *ux = 0; *uy = 0; return; }
    decode(best, ux, uy);
}

/* The fetch rule: 1 = prev's sample alone, 2 = curr's alone, 0 = the rule does not decide. */
static int fetch_rule(const uint8_t *mask, int W, int H, float Px, float Py, float Cx, float Cy) {
#ifdef OV_MUTANT_RULE_LRINT
    const int px = clampi((int)lrintf(Px), 0, W - 1), py = clampi((int)lrintf(Py), 0, H - 1);
    const int cx = clampi((int)lrintf(Cx), 0, W - 1), cy = clampi((int)lrintf(Cy), 0, H - 1);
#else
    const int px = clampi((int)floorf(Px), 0, W - 1), py = clampi((int)floorf(Py), 0, H - 1);
    const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
#endif
    const int sp = mask[(size_t)py * W + px] != 0, sc = mask[(size_t)cy * W + cx] != 0;
    if (sp && !sc) return 2;                                   /* the content is hidden under the overlay in prev */
    if (sc && !sp) return 1;
    return 0;
}

void ov_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint8_t *mask, const uint32_t *K, int W, int H,
               float t, int match_sad, int x0, int y0, int x1, int y1, uint8_t *out) {
    const float s = 1.0f - t;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            uint8_t *o = out + ((size_t)(y - y0) * (x1 - x0) + (x - x0)) * 4;
            const uint32_t key = K[(size_t)y * W + x];
            if (key == STATIC) {                               /* the two texels directly: no positions */
                const uint8_t *p = prev + ((size_t)y * W + x) * 4, *c = curr + ((size_t)y * W + x) * 4;
#ifdef OV_MUTANT_STATIC_CURR
                const vec4 m = {unorm(c[0]), unorm(c[1]), unorm(c[2]), unorm(c[3])};
                (void)p;
#else
                const vec4 m = {mixf(unorm(p[0]), unorm(c[0]), t), mixf(unorm(p[1]), unorm(c[1]), t),
                                mixf(unorm(p[2]), unorm(c[2]), t), mixf(unorm(p[3]), unorm(c[3]), t)};
#endif
                store(o, m);
                continue;
            }
            int ux, uy;
            const int hole = key == HOLE;
            if (hole) fill_vector_past_static(K, W, H, x, y, &ux, &uy);
            else decode(key, &ux, &uy);
            const float Px = ((float)x + 0.5f) + (float)ux * t, Py = ((float)y + 0.5f) + (float)uy * t;
            const float Cx = ((float)x + 0.5f) - (float)ux * s, Cy = ((float)y + 0.5f) - (float)uy * s;
            const vec4 Pv = bilinear_px(prev, W, H, Px, Py), Cv = bilinear_px(curr, W, H, Cx, Cy);
#ifndef OV_MUTANT_RULE_AFTER_HOLE
            const int rule = fetch_rule(mask, W, H, Px, Py, Cx, Cy);
            if (rule == 2) { store(o, Cv); continue; }
            if (rule == 1) { store(o, Pv); continue; }
#endif
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                if (!matched(prev, curr, mv, W, H, cx, cy, match_sad)) { store(o, Cv); continue; }     /* revealed */
                const int8_t *v = mv + ((size_t)cy * W + cx) * 2;
                if (v[0] != ux || v[1] != uy) { store(o, Pv); continue; }                              /* covered */
            }
#ifdef OV_MUTANT_RULE_AFTER_HOLE
            const int rule = fetch_rule(mask, W, H, Px, Py, Cx, Cy);
            if (rule == 2) { store(o, Cv); continue; }
            if (rule == 1) { store(o, Pv); continue; }
#endif
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}
