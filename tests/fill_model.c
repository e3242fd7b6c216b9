/* CPU model of the fill plane (lfg_hole_fill_plane, lfg_set_hole_reach; include/linuxfg_hip.h): the plane by plain loops from
 * its definition, and the sampling steps of lfg_interpolate_compensated, _masked and _bidirectional with a hole's vector read
 * from a plane.  Built with the system C compiler and -ffp-contract=off by tests/fill_model.py.  The library's helpers, the
 * gate, the key, its decode and the end of the sampling are tests/compensated_model.h's; its walk (fill_vector) is not used
 * here: this file is what replaces it.  The three sampling steps restate mc_model.c, overlay_model.c and bidir_model.c with
 * that one difference (tests/test_fill_model.py holds them to each other byte for byte at reach 16).
 *
 * K and the plane are tight: rows of W words.  Frames, vectors and masks as in the three models.
 *
 * Mutants, for the test of the tests alone (tests/test_fill_model.py: a plane case must tell each of them from the model);
 * with no such macro defined this file is the model:
 *   FILL_MUTANT_STRICT_REACH      `<` for `<=` at the reach;
 *   FILL_MUTANT_PROJECTION_MIN    the minimum taken over the stored (projection) keys instead of over the walk order;
 *   FILL_MUTANT_STATIC_DONOR      a static word is a donor even with pass_static;
 *   FILL_MUTANT_SELF_DONOR        the pixel itself counts, at distance 0;
 *   FILL_MUTANT_COLUMN_OF_PLANE   two passes, the column pass scanning the row pass's plane instead of K. */
#include "compensated_model.h"

#define STATIC 0u

static int donor(uint32_t word, int pass_static) {
#ifdef FILL_MUTANT_STATIC_DONOR
    (void)pass_static;
    return word != HOLE;
#else
    return word != HOLE && !(pass_static && word == STATIC);
#endif
}

#ifdef FILL_MUTANT_STRICT_REACH
#define WITHIN(j, reach) ((j) < (reach))
#else
#define WITHIN(j, reach) ((j) <= (reach))
#endif
#ifdef FILL_MUTANT_SELF_DONOR
#define FIRST_STEP 0
#else
#define FIRST_STEP 1
#endif

/* the nearest donor from (x, y) along (sx, sy), as its walk-order key; HOLE if the image or the reach ends first */
static uint32_t nearest(const uint32_t *K, int W, int H, int x, int y, int sx, int sy, int reach, int pass_static) {
    for (int j = FIRST_STEP; WITHIN(j, reach); ++j) {
        const int nx = x + sx * j, ny = y + sy * j;
        if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
        if (donor(K[(size_t)ny * W + nx], pass_static)) {
#ifdef FILL_MUTANT_PROJECTION_MIN
            return K[(size_t)ny * W + nx];
#else
            return walk_order(K[(size_t)ny * W + nx]);
#endif
        }
    }
    return HOLE;
}

void fill_plane(const uint32_t *K, int W, int H, int reach, int pass_static, uint32_t *plane) {
    static const int dir[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
#ifdef FILL_MUTANT_COLUMN_OF_PLANE
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint32_t best = HOLE;
            for (int k = 0; k < 2; ++k) {
                const uint32_t n = nearest(K, W, H, x, y, dir[k][0], dir[k][1], reach, pass_static);
                if (n < best) best = n;
            }
            plane[(size_t)y * W + x] = best;
        }
    uint32_t *rows = malloc((size_t)W * H * sizeof *rows);
    for (size_t i = 0; i < (size_t)W * H; ++i) rows[i] = plane[i];
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 2; k < 4; ++k)
                for (int j = 1; j <= reach; ++j) {
                    const int ny = y + dir[k][1] * j;
                    if (ny < 0 || ny >= H) break;
                    if (rows[(size_t)ny * W + x] == HOLE) continue;
                    if (rows[(size_t)ny * W + x] < plane[(size_t)y * W + x]) plane[(size_t)y * W + x] = rows[(size_t)ny * W + x];
                    break;
                }
    free(rows);
#else
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint32_t best = HOLE;
            for (int k = 0; k < 4; ++k) {
                const uint32_t n = nearest(K, W, H, x, y, dir[k][0], dir[k][1], reach, pass_static);
                if (n < best) best = n;
            }
#ifdef FILL_MUTANT_PROJECTION_MIN
            if (best != HOLE) best = walk_order(best);
#endif
            plane[(size_t)y * W + x] = best;
        }
#endif
}

/* a hole's vector from the plane: the hole word decodes as (0, 0) */
static void from_plane(const uint32_t *plane, int W, int x, int y, int *ux, int *uy) {
    const uint32_t best = plane[(size_t)y * W + x];
    if (best == HOLE) { *ux = 0; *uy = 0; return; }
    decode(best, ux, uy);
}

/* mc_model.c: mc_sample */
void fill_mc_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint32_t *K, const uint32_t *plane, int W, int H,
                    float t, int match_sad, uint8_t *out) {
    const float s = 1.0f - t;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint8_t *o = out + ((size_t)y * W + x) * 4;
            const uint32_t key = K[(size_t)y * W + x];
            int ux, uy;
            const int hole = key == HOLE;
            if (hole) from_plane(plane, W, x, y, &ux, &uy);
            else decode(key, &ux, &uy);
            const float Px = ((float)x + 0.5f) + (float)ux * t, Py = ((float)y + 0.5f) + (float)uy * t;
            const float Cx = ((float)x + 0.5f) - (float)ux * s, Cy = ((float)y + 0.5f) - (float)uy * s;
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

/* overlay_model.c: ov_sample, the plane made with pass_static = 1 */
void fill_ov_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *mv, const uint8_t *mask, const uint32_t *K,
                    const uint32_t *plane, int W, int H, float t, int match_sad, uint8_t *out) {
    const float s = 1.0f - t;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint8_t *o = out + ((size_t)y * W + x) * 4;
            const uint32_t key = K[(size_t)y * W + x];
            if (key == STATIC) {
                const uint8_t *p = prev + ((size_t)y * W + x) * 4, *c = curr + ((size_t)y * W + x) * 4;
                const vec4 m = {mixf(unorm(p[0]), unorm(c[0]), t), mixf(unorm(p[1]), unorm(c[1]), t),
                                mixf(unorm(p[2]), unorm(c[2]), t), mixf(unorm(p[3]), unorm(c[3]), t)};
                store(o, m);
                continue;
            }
            int ux, uy;
            const int hole = key == HOLE;
            if (hole) from_plane(plane, W, x, y, &ux, &uy);
            else decode(key, &ux, &uy);
            const float Px = ((float)x + 0.5f) + (float)ux * t, Py = ((float)y + 0.5f) + (float)uy * t;
            const float Cx = ((float)x + 0.5f) - (float)ux * s, Cy = ((float)y + 0.5f) - (float)uy * s;
            const vec4 Pv = bilinear_px(prev, W, H, Px, Py), Cv = bilinear_px(curr, W, H, Cx, Cy);
            const int px = clampi((int)floorf(Px), 0, W - 1), py = clampi((int)floorf(Py), 0, H - 1);
            const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
            const int sp = mask[(size_t)py * W + px] != 0, sc = mask[(size_t)cy * W + cx] != 0;
            if (sp && !sc) { store(o, Cv); continue; }                 /* the fetch rule */
            if (sc && !sp) { store(o, Pv); continue; }
            if (hole) {
                if (!matched(prev, curr, mv, W, H, cx, cy, match_sad)) { store(o, Cv); continue; }     /* revealed */
                const int8_t *v = mv + ((size_t)cy * W + cx) * 2;
                if (v[0] != ux || v[1] != uy) { store(o, Pv); continue; }                              /* covered */
            }
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}

/* bidir_model.c: consistent, confirmed_f, confirmed_b, bidir_sample */
static int consistent(const int8_t *a, const int8_t *b, int W, int H, int qx, int qy, int tolerance) {
    const int ax = a[((size_t)qy * W + qx) * 2], ay = a[((size_t)qy * W + qx) * 2 + 1];
    const int rx = qx + ax, ry = qy + ay;
    if (rx < 0 || rx >= W || ry < 0 || ry >= H) return 0;
    return abs(ax + b[((size_t)ry * W + rx) * 2]) + abs(ay + b[((size_t)ry * W + rx) * 2 + 1]) <= tolerance;
}

static int confirmed_f(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, int W, int H, int qx, int qy,
                       int match_sad, int tolerance) {
    return gate(curr, prev, fwd, W, H, qx, qy, match_sad) && consistent(fwd, bwd, W, H, qx, qy, tolerance);
}

static int confirmed_b(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, int W, int H, int px, int py,
                       int match_sad, int tolerance) {
    if (bwd[((size_t)py * W + px) * 2] == -128 || bwd[((size_t)py * W + px) * 2 + 1] == -128) return 0;
    return gate(prev, curr, bwd, W, H, px, py, match_sad) && consistent(bwd, fwd, W, H, px, py, tolerance);
}

void fill_bidir_sample(const uint8_t *prev, const uint8_t *curr, const int8_t *fwd, const int8_t *bwd, const uint32_t *K,
                       const uint32_t *plane, int W, int H, float t, int match_sad, int tolerance, uint8_t *out) {
    const float s = 1.0f - t;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint8_t *o = out + ((size_t)y * W + x) * 4;
            const uint32_t key = K[(size_t)y * W + x];
            int ux, uy;
            const int hole = key == HOLE;
            if (hole) from_plane(plane, W, x, y, &ux, &uy);
            else decode(key, &ux, &uy);
            const float Px = ((float)x + 0.5f) + (float)ux * t, Py = ((float)y + 0.5f) + (float)uy * t;
            const float Cx = ((float)x + 0.5f) - (float)ux * s, Cy = ((float)y + 0.5f) - (float)uy * s;
            const vec4 Pv = bilinear_px(prev, W, H, Px, Py), Cv = bilinear_px(curr, W, H, Cx, Cy);
            if (hole) {
                const int cx = clampi((int)floorf(Cx), 0, W - 1), cy = clampi((int)floorf(Cy), 0, H - 1);
                const int px = clampi((int)floorf(Px), 0, W - 1), py = clampi((int)floorf(Py), 0, H - 1);
                const int8_t *f = fwd + ((size_t)cy * W + cx) * 2, *b = bwd + ((size_t)py * W + px) * 2;
                const int cbad = confirmed_f(prev, curr, fwd, bwd, W, H, cx, cy, match_sad, tolerance) && (f[0] != ux || f[1] != uy);
                const int pbad = confirmed_b(prev, curr, fwd, bwd, W, H, px, py, match_sad, tolerance) && (-b[0] != ux || -b[1] != uy);
                if (cbad && !pbad) { store(o, Pv); continue; }                                        /* covered in curr */
                if (pbad && !cbad) { store(o, Cv); continue; }                                        /* revealed in curr */
            }
            store_inside_or_blend(o, Pv, Cv, Px, Py, Cx, Cy, W, H, t);
        }
}
