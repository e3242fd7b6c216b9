/* CPU model of lfg_motion_pyramid (include/linuxfg_hip.h), integer arithmetic as the header fixes it.  Built with the
 * system C compiler by tests/pyramid_model.py.
 *
 * pyramid_level: one reduce step.  pyramid_vectors: the vectors of one level over a rectangle of pixels, from the images of
 * that level and (refinement) the parent level's vectors over the rectangle's parents. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

void pyramid_level(const uint8_t *src, int Ws, int Hs, uint8_t *dst, int Wd, int Hd) {
    for (int y = 0; y < Hd; ++y)
        for (int x = 0; x < Wd; ++x) {
            const int x0 = 2 * x, y0 = 2 * y, x1 = 2 * x + 1 < Ws ? 2 * x + 1 : Ws - 1, y1 = 2 * y + 1 < Hs ? 2 * y + 1 : Hs - 1;
            for (int c = 0; c < 4; ++c) {
                const int s = src[((size_t)y0 * Ws + x0) * 4 + c] + src[((size_t)y0 * Ws + x1) * 4 + c] +
                              src[((size_t)y1 * Ws + x0) * 4 + c] + src[((size_t)y1 * Ws + x1) * 4 + c];
                dst[((size_t)y * Wd + x) * 4 + c] = (uint8_t)((s + 2) >> 2);
            }
        }
}

static inline uint64_t key_of(uint32_t cost, int vx, int vy) {
    return ((uint64_t)cost << 32) | ((uint64_t)(vx * vx + vy * vy) << 16) | ((uint64_t)(vy + 128) << 8) | (uint64_t)(vx + 128);
}

static inline uint32_t texel_sad(const uint8_t *a, const uint8_t *b) {
    uint32_t s = 0;
    for (int c = 0; c < 4; ++c) s += (uint32_t)abs((int)a[c] - (int)b[c]);
    return s;
}

static uint32_t cost_at(const uint8_t *prev, const uint8_t *curr, int W, int H, int px, int py, int vx, int vy) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    uint32_t s = 0;
    for (int by = -4; by < 4; ++by) {
        const int qy = py + by;
        if (qy < 0 || qy >= H) continue;
        for (int bx = -4; bx < 4; ++bx) {
            const int qx = px + bx;
            if (qx < 0 || qx >= W) continue;
            const int sx = qx + vx, sy = qy + vy;
            const uint8_t *p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? prev + ((size_t)sy * W + sx) * 4 : zero;
            s += texel_sad(curr + ((size_t)qy * W + qx) * 4, p);
        }
    }
    return s;
}

/* Vectors (x, y as int8 pairs) of level images prev / curr (W x H, tight RGBA8) for pixels [x0, x1) x [y0, y1), written to
 * out[(y - y0) * (x1 - x0) + (x - x0)].  parent == NULL: the full search over [-R, R]^2 (R = coarse radius).  Otherwise
 * parent holds the level above's vectors for pixels [x0 / 2, ...) x [y0 / 2, ...) in rows of pw, and the candidates are
 * 2 * parent + [-R, R]^2 (R = refine radius) and (0,0). */
void pyramid_vectors(const uint8_t *prev, const uint8_t *curr, int W, int H, int x0, int y0, int x1, int y1,
                     const int8_t *parent, int pw, int R, int8_t *out) {
    const int rw = x1 - x0, rh = y1 - y0;
    if (!parent) {
        /* per candidate: texel SADs over the rectangle's blocks, then 8 x 8 box sums, separably */
        const int ex0 = x0 - 4, ey0 = y0 - 4, ew = rw + 7, eh = rh + 7;
        uint32_t *d = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)ew * eh);
        uint32_t *hs = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)rw * eh);
        uint64_t *best = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)rw * rh);
        for (size_t i = 0; i < (size_t)rw * rh; ++i) best[i] = ~0ull;
        static const uint8_t zero[4] = {0, 0, 0, 0};
        for (int vy = -R; vy <= R; ++vy)
            for (int vx = -R; vx <= R; ++vx) {
                for (int j = 0; j < eh; ++j)
                    for (int i = 0; i < ew; ++i) {
                        const int qx = ex0 + i, qy = ey0 + j;
                        uint32_t v = 0;
                        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
                            const int sx = qx + vx, sy = qy + vy;
                            const uint8_t *p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? prev + ((size_t)sy * W + sx) * 4 : zero;
                            v = texel_sad(curr + ((size_t)qy * W + qx) * 4, p);
                        }
                        d[(size_t)j * ew + i] = v;
                    }
                for (int j = 0; j < eh; ++j)
                    for (int i = 0; i < rw; ++i) {
                        uint32_t s = 0;
                        for (int k = 0; k < 8; ++k) s += d[(size_t)j * ew + i + k];
                        hs[(size_t)j * rw + i] = s;
                    }
                for (int j = 0; j < rh; ++j)
                    for (int i = 0; i < rw; ++i) {
                        uint32_t s = 0;
                        for (int k = 0; k < 8; ++k) s += hs[(size_t)(j + k) * rw + i];
                        const uint64_t key = key_of(s, vx, vy);
                        if (key < best[(size_t)j * rw + i]) best[(size_t)j * rw + i] = key;
                    }
            }
        for (size_t i = 0; i < (size_t)rw * rh; ++i) {
            out[2 * i] = (int8_t)((int)(best[i] & 0xff) - 128);
            out[2 * i + 1] = (int8_t)((int)((best[i] >> 8) & 0xff) - 128);
        }
        free(d); free(hs); free(best);
        return;
    }
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            const int8_t *pv = parent + ((size_t)(y / 2 - y0 / 2) * pw + (x / 2 - x0 / 2)) * 2;
            const int cx = 2 * pv[0], cy = 2 * pv[1];
            uint64_t best = key_of(cost_at(prev, curr, W, H, x, y, 0, 0), 0, 0);
            for (int dy = -R; dy <= R; ++dy)
                for (int dx = -R; dx <= R; ++dx) {
                    const int vx = cx + dx, vy = cy + dy;
                    const uint64_t key = key_of(cost_at(prev, curr, W, H, x, y, vx, vy), vx, vy);
                    if (key < best) best = key;
                }
            int8_t *o = out + ((size_t)(y - y0) * rw + (x - x0)) * 2;
            o[0] = (int8_t)((int)(best & 0xff) - 128);
            o[1] = (int8_t)((int)((best >> 8) & 0xff) - 128);
        }
}
