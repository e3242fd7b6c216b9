// Coarse-to-fine block matcher (lfg_motion_pyramid, include/linuxfg_hip.h).  No reference counterpart: shaders/motion.comp is
// one +-16 full search.  The algorithm is integer-only and fixed in the header; tests/pyramid_model.py restates it in numpy.
//
//   pyramid_reduce_kernel   level k of prev and curr from level k - 1: 2 x 2 box, (sum + 2) >> 2 per channel, edges clamped
//   pyramid_search_kernel   level L: every v in [-Rc, Rc]^2
//   pyramid_refine_kernel   level k < L: 2 * (parent's vector) + [-Rr, Rr]^2, and (0,0)
//
// Both matchers give each lane one 2 x 2 quad of output pixels.  The four 8 x 8 blocks of a quad (block = p + [-4, 3]^2)
// lie in one 9 x 9 window of curr, which the lane keeps in registers; per candidate it takes 81 packed-RGBA SADs
// (v_sad_u8) against prev, one row sum of 8 per row, the right neighbour's by one add and one subtract, and the four costs
// as sums of 8 row sums: 81 SADs + ~40 adds for four (pixel, candidate) pairs instead of 256 SADs.  A wave covers an 8 x 8 tile
// of quads (16 x 16 pixels).  The prev values a candidate needs come from LDS: in the search kernel one window around the tile
// serves every candidate (all quads share the candidate set) and eight waves split the candidates; in the refine kernel each
// quad has its own window around twice its parent's vector, (9 + 2 Rr)^2 texels, staged once and read by all its
// (2 Rr + 1)^2 candidates.  Measured cost and what bounds it: DESIGN.md section 4.6.
//
// Order of candidates: the smallest key (C, vx^2 + vy^2, vy, vx), one uint64 -- total, so neither tiling nor evaluation
// order changes a result.  No data-dependent exits: every call costs the same on every content.
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_vector_word.hpp"

namespace lfg {
namespace {

constexpr int kQ = 8;                  // quads per tile side: a wave = 8 x 8 quads = 16 x 16 pixels
constexpr int kTile = 2 * kQ;
constexpr int kWin = 9;                // a quad's curr window side (8 + 1)
constexpr int kSearchWaves = 8;        // waves of a search workgroup

// Nine consecutive dwords of an LDS row, starting at an index whose parity is ODD (wave-uniform): four 8-byte reads and one
// 4-byte read instead of nine 4-byte ones (ds_read_b64 moves twice the bytes per LDS cycle).
template <int ODD>
__device__ __forceinline__ void lds_row9(const uint32_t *row, uint32_t (&p)[kWin]) {
    if (ODD) {
        p[0] = row[0];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint2 t = *reinterpret_cast<const uint2 *>(row + 1 + 2 * i);
            p[1 + 2 * i] = t.x; p[2 + 2 * i] = t.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint2 t = *reinterpret_cast<const uint2 *>(row + 2 * i);
            p[2 * i] = t.x; p[2 * i + 1] = t.y;
        }
        p[8] = row[8];
    }
}

// The four costs of one candidate for a quad.  c: the quad's curr window; win + start: the prev texel under c[0] for this
// candidate, rows `pitch` apart.  EDGE: curr texels outside the image (valid bits clear) add nothing.  cost[j * 2 + i]: child
// (i, j) of the quad.
template <bool EDGE, int ODD>
__device__ __forceinline__ void quad_costs(const uint32_t (&c)[kWin * kWin], uint32_t colOk, uint32_t rowOk,
                                           const uint32_t *win, int pitch, uint32_t (&cost)[4]) {
    uint32_t top0 = 0u, top1 = 0u, r0Left = 0u, r0Right = 0u, r8Left = 0u, r8Right = 0u;
#pragma unroll
    for (int r = 0; r < kWin; ++r) {
        uint32_t p[kWin];
        lds_row9<ODD>(win + r * pitch, p);
        uint32_t d[kWin];
#pragma unroll
        for (int i = 0; i < kWin; ++i) {
            d[i] = __builtin_amdgcn_sad_u8(c[r * kWin + i], p[i], 0u);
            if (EDGE) d[i] = (((colOk >> i) & (rowOk >> r)) & 1u) ? d[i] : 0u;
        }
        uint32_t left = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) left += d[i];
        const uint32_t right = left - d[0] + d[8];
        top0 += left; top1 += right;                   // rows 0 .. 8
        if (r == 0) { r0Left = left; r0Right = right; }
        if (r == 8) { r8Left = left; r8Right = right; }
    }
    cost[0] = top0 - r8Left;  cost[1] = top1 - r8Right;       // rows 0 .. 7
    cost[2] = top0 - r0Left;  cost[3] = top1 - r0Right;       // rows 1 .. 8
}

struct QuadCurr {
    uint32_t c[kWin * kWin];
    uint32_t colOk, rowOk;             // bit i: window column / row i lies inside the image
};

// The quad's 9 x 9 curr window: texels (2X - 4 .. 2X + 4, 2Y - 4 .. 2Y + 4).
__device__ __forceinline__ void load_quad_curr(QuadCurr &q, const uint8_t *curr, size_t pitch, int W, int H, int X, int Y) {
    q.colOk = q.rowOk = 0u;
#pragma unroll
    for (int i = 0; i < kWin; ++i) {
        const int x = 2 * X - 4 + i, y = 2 * Y - 4 + i;
        q.colOk |= (x >= 0 && x < W) ? 1u << i : 0u;
        q.rowOk |= (y >= 0 && y < H) ? 1u << i : 0u;
    }
#pragma unroll
    for (int r = 0; r < kWin; ++r)
#pragma unroll
        for (int i = 0; i < kWin; ++i) q.c[r * kWin + i] = texel_or_zero_branch(curr, pitch, 2 * X - 4 + i, 2 * Y - 4 + r, W, H);
}

__device__ __forceinline__ void keep_min(uint64_t &best, uint32_t cost, uint32_t rank) {
    const uint64_t k = ((uint64_t)cost << 32) | rank;
    best = k < best ? k : best;
}

__device__ __forceinline__ void store_quad(uint8_t *mv, size_t pitch, int W, int H, int X, int Y, const uint64_t (&best)[4]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int x = 2 * X + i, y = 2 * Y + j;
            if (x >= W || y >= H) continue;
            const Mv v = mv_order_decode((uint32_t)best[j * 2 + i]);
            *reinterpret_cast<uint16_t *>(mv + (size_t)y * pitch + (size_t)x * 2u) = mv_word(v.x, v.y);
        }
}

// Is the 9 x 9 curr window of every quad of the wave's tile inside the image?  (wave-uniform)
__device__ __forceinline__ bool tile_inside(int x0, int y0, int W, int H) {
    return x0 - 4 >= 0 && y0 - 4 >= 0 && x0 + kTile + 3 < W && y0 + kTile + 3 < H;
}

// Every v in [-Rc, Rc]^2 whose vy is vy0 + k * step; base: the LDS texel under c[0] for v = (0,0), rows `side` apart.
template <bool EDGE>
__device__ __forceinline__ void search_all(const QuadCurr &q, const uint32_t *base, int side, int Rc, int vy0, int step, uint64_t (&best)[4]) {
    for (int vy = vy0; vy <= Rc; vy += step) {
        const uint32_t *row = base + vy * side;
        for (int vx = -Rc; vx <= Rc; ++vx) {
            uint32_t cost[4];
            if ((vx + Rc) & 1) quad_costs<EDGE, 1>(q.c, q.colOk, q.rowOk, row + vx, side, cost);
            else quad_costs<EDGE, 0>(q.c, q.colOk, q.rowOk, row + vx, side, cost);
            const uint32_t rank = mv_order_key(vx, vy);
#pragma unroll
            for (int k = 0; k < 4; ++k) keep_min(best[k], cost[k], rank);
        }
    }
}

// (cx, cy) + [-Rr, Rr]^2 from the quad's own window (its texel 0 lies under c[0] for d = (-Rr, -Rr); rows `side` apart).
template <bool EDGE>
__device__ __forceinline__ void refine_all(const QuadCurr &q, const uint32_t *win, int side, int Rr, int cx, int cy, uint64_t (&best)[4]) {
    for (int dy = -Rr; dy <= Rr; ++dy) {
        const uint32_t *row = win + (dy + Rr) * side;
        for (int dx = -Rr; dx <= Rr; ++dx) {
            uint32_t cost[4];
            if ((dx + Rr) & 1) quad_costs<EDGE, 1>(q.c, q.colOk, q.rowOk, row + dx + Rr, side, cost);
            else quad_costs<EDGE, 0>(q.c, q.colOk, q.rowOk, row + dx + Rr, side, cost);
            const uint32_t rank = mv_order_key(cx + dx, cy + dy);
#pragma unroll
            for (int k = 0; k < 4; ++k) keep_min(best[k], cost[k], rank);
        }
    }
}

}  // namespace

// One level of both frames.  src: level k - 1 (pitched), dst: level k (tight rows).  blockIdx.y: 0 prev, 1 curr.
__global__ __launch_bounds__(256) void pyramid_reduce_kernel(const uint8_t *__restrict__ prevSrc, size_t prevPitch,
                                                             const uint8_t *__restrict__ currSrc, size_t currPitch, int Ws, int Hs,
                                                             uint8_t *__restrict__ prevDst, uint8_t *__restrict__ currDst, int Wd, int Hd) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)Wd * (size_t)Hd) return;
    const uint8_t *src = blockIdx.y ? currSrc : prevSrc;
    const size_t pitch = blockIdx.y ? currPitch : prevPitch;
    uint8_t *dst = blockIdx.y ? currDst : prevDst;
    const int y = (int)(i / (size_t)Wd), x = (int)(i - (size_t)y * (size_t)Wd);
    const int x0 = 2 * x, y0 = 2 * y, x1 = min(2 * x + 1, Ws - 1), y1 = min(2 * y + 1, Hs - 1);
    const uint32_t a = *reinterpret_cast<const uint32_t *>(src + (size_t)y0 * pitch + (size_t)x0 * 4u);
    const uint32_t b = *reinterpret_cast<const uint32_t *>(src + (size_t)y0 * pitch + (size_t)x1 * 4u);
    const uint32_t c = *reinterpret_cast<const uint32_t *>(src + (size_t)y1 * pitch + (size_t)x0 * 4u);
    const uint32_t d = *reinterpret_cast<const uint32_t *>(src + (size_t)y1 * pitch + (size_t)x1 * 4u);
    // channels 0 and 2 / 1 and 3 in 16-bit halves: four bytes plus 2 stay below 2^11
    const uint32_t even = (a & 0x00FF00FFu) + (b & 0x00FF00FFu) + (c & 0x00FF00FFu) + (d & 0x00FF00FFu) + 0x00020002u;
    const uint32_t odd = ((a >> 8) & 0x00FF00FFu) + ((b >> 8) & 0x00FF00FFu) + ((c >> 8) & 0x00FF00FFu) + ((d >> 8) & 0x00FF00FFu) + 0x00020002u;
    *reinterpret_cast<uint32_t *>(dst + i * 4u) = ((even >> 2) & 0x00FF00FFu) | (((odd >> 2) & 0x00FF00FFu) << 8);
}

// Level L: the full +-Rc search.  A workgroup per 16 x 16 tile, its kSearchWaves waves on interleaved rows of candidates (one
// wave per tile left most SIMDs idle at 1080p: 510 tiles), the per-pixel minima combined through LDS.  LDS: prev over the
// tile's curr windows widened by Rc on each side, (24 + 2 Rc)^2 texels (outside the image: 0).
__global__ __launch_bounds__(64 * kSearchWaves) void pyramid_search_kernel(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ curr, size_t pitch,
                                                            int W, int H, int Rc, uint8_t *__restrict__ mv, size_t mvPitch) {
    extern __shared__ uint32_t sPrev[];
    const int side = kTile + 8 + 2 * Rc;                 // even
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int ox = x0 - 4 - Rc, oy = y0 - 4 - Rc;
    for (int i = (int)threadIdx.x; i < side * side; i += 64 * kSearchWaves) {
        const int r = i / side, col = i - r * side;
        sPrev[i] = texel_or_zero_branch(prev, pitch, ox + col, oy + r, W, H);
    }
    const int lane = (int)threadIdx.x % 64, wave = (int)threadIdx.x / 64;
    const int qx = lane % kQ, qy = lane / kQ;
    const int X = (int)blockIdx.x * kQ + qx, Y = (int)blockIdx.y * kQ + qy;
    QuadCurr q;
    load_quad_curr(q, curr, pitch, W, H, X, Y);
    __syncthreads();
    uint64_t best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    const uint32_t *base = sPrev + (2 * qy + Rc) * side + 2 * qx + Rc;       // under c[0] for v = (0,0)
    if (tile_inside(x0, y0, W, H)) search_all<false>(q, base, side, Rc, wave - Rc, kSearchWaves, best);
    else search_all<true>(q, base, side, Rc, wave - Rc, kSearchWaves, best);
    __shared__ uint64_t sBest[kSearchWaves - 1][4][64];
    if (wave > 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) sBest[wave - 1][k][lane] = best[k];
    __syncthreads();
    if (wave > 0) return;
    for (int w = 0; w < kSearchWaves - 1; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = sBest[w][k][lane] < best[k] ? sBest[w][k][lane] : best[k];
    if (2 * X < W && 2 * Y < H) store_quad(mv, mvPitch, W, H, X, Y, best);
}

// Level k < L.  One wave per 16 x 16 tile; each lane stages the prev window of its quad's candidate set, 2 * parent +
// [-Rr, Rr]^2: (9 + 2 Rr)^2 texels in rows of 10 + 2 Rr (an even row pitch keeps the 8-byte reads aligned).
__global__ __launch_bounds__(64) void pyramid_refine_kernel(const uint8_t *__restrict__ prev, size_t prevPitch,
                                                            const uint8_t *__restrict__ curr, size_t currPitch, int W, int H,
                                                            const uint8_t *__restrict__ parent, size_t parentPitch, int Rr,
                                                            uint8_t *__restrict__ mv, size_t mvPitch) {
    extern __shared__ uint32_t sWin[];
    const int side = kWin + 2 * Rr, pitch = side + 1;
    const int qx = (int)threadIdx.x % kQ, qy = (int)threadIdx.x / kQ;
    const int X = (int)blockIdx.x * kQ + qx, Y = (int)blockIdx.y * kQ + qy;
    const int Wp = (W + 1) / 2, Hp = (H + 1) / 2;
    int cx = 0, cy = 0;
    if (X < Wp && Y < Hp) {
        const Mv pv = mv_unpack(*reinterpret_cast<const uint16_t *>(parent + (size_t)Y * parentPitch + (size_t)X * 2u));
        cx = 2 * pv.x, cy = 2 * pv.y;
    }
    QuadCurr q;
    load_quad_curr(q, curr, currPitch, W, H, X, Y);
    // Each lane reads only what it wrote itself: no barrier.  First (0,0) -- it need not lie in the candidate window -- through
    // the same region, then the window.
    uint32_t *win = sWin + threadIdx.x * (side * pitch);
    uint64_t best[4];
    {
        for (int r = 0; r < kWin; ++r)
            for (int i = 0; i < kWin; ++i) win[r * pitch + i] = texel_or_zero_branch(prev, prevPitch, 2 * X - 4 + i, 2 * Y - 4 + r, W, H);
        uint32_t cost[4];
        quad_costs<true, 0>(q.c, q.colOk, q.rowOk, win, pitch, cost);
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = ((uint64_t)cost[k] << 32) | mv_order_key(0, 0);
    }
    const int wx = 2 * X - 4 + cx - Rr, wy = 2 * Y - 4 + cy - Rr;
    for (int r = 0; r < side; ++r)
        for (int i = 0; i < side; ++i) win[r * pitch + i] = texel_or_zero_branch(prev, prevPitch, wx + i, wy + r, W, H);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    if (tile_inside(x0, y0, W, H)) refine_all<false>(q, win, pitch, Rr, cx, cy, best);
    else refine_all<true>(q, win, pitch, Rr, cx, cy, best);
    if (2 * X < W && 2 * Y < H) store_quad(mv, mvPitch, W, H, X, Y, best);
}

size_t pyramid_workspace_bytes(uint32_t width, uint32_t height, int levels, PyramidLayout *layout) {
    PyramidLayout l{};
    l.levels = levels;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255u) & ~(size_t)255u; return at; };
    uint32_t w = width, h = height;
    for (int k = 1; k <= levels; ++k) {
        w = (w + 1u) / 2u; h = (h + 1u) / 2u;
        l.w[k] = w; l.h[k] = h;
        l.prev[k] = take((size_t)w * h * 4u);
        l.curr[k] = take((size_t)w * h * 4u);
        l.mv[k] = take((size_t)w * h * 2u);
    }
    l.w[0] = width; l.h[0] = height;
    l.total = off;
    if (layout) *layout = l;
    return off;
}

hipError_t launch_motion_pyramid(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                 int levels, int coarseRadius, int refineRadius, uint8_t *ws, const PyramidLayout &l) {
    // the pyramids
    for (int k = 1; k <= levels; ++k) {
        const uint8_t *ps = k == 1 ? (const uint8_t *)prev.data : ws + l.prev[k - 1];
        const uint8_t *cs = k == 1 ? (const uint8_t *)curr.data : ws + l.curr[k - 1];
        const size_t pp = k == 1 ? prev.pitch : (size_t)l.w[k - 1] * 4u, cp = k == 1 ? curr.pitch : (size_t)l.w[k - 1] * 4u;
        const size_t n = (size_t)l.w[k] * l.h[k];
        const dim3 grid((unsigned)((n + 255u) / 256u), 2);
        hipLaunchKernelGGL(pyramid_reduce_kernel, grid, dim3(256), 0, s, ps, pp, cs, cp, (int)l.w[k - 1], (int)l.h[k - 1],
                           ws + l.prev[k], ws + l.curr[k], (int)l.w[k], (int)l.h[k]);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // level L: the full search
    {
        const int W = (int)l.w[levels], H = (int)l.h[levels];
        const dim3 grid((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile));
        const int side = kTile + 8 + 2 * coarseRadius;
        const size_t lds = (size_t)side * side * 4u;
        hipLaunchKernelGGL(pyramid_search_kernel, grid, dim3(64 * kSearchWaves), lds, s, ws + l.prev[levels], ws + l.curr[levels],
                           (size_t)W * 4u, W, H, coarseRadius, ws + l.mv[levels], (size_t)W * 2u);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // levels L - 1 .. 0
    for (int k = levels - 1; k >= 0; --k) {
        const int W = (int)l.w[k], H = (int)l.h[k];
        const uint8_t *p = k == 0 ? (const uint8_t *)prev.data : ws + l.prev[k];
        const uint8_t *c = k == 0 ? (const uint8_t *)curr.data : ws + l.curr[k];
        const size_t pp = k == 0 ? prev.pitch : (size_t)W * 4u, cp = k == 0 ? curr.pitch : (size_t)W * 4u;
        uint8_t *out = k == 0 ? (uint8_t *)mv.data : ws + l.mv[k];
        const size_t op = k == 0 ? mv.pitch : (size_t)W * 2u;
        const dim3 grid((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile));
        const int side = kWin + 2 * refineRadius;
        const size_t lds = (size_t)64 * side * (side + 1) * 4u;
        hipLaunchKernelGGL(pyramid_refine_kernel, grid, dim3(64), lds, s, p, pp, c, cp, W, H, ws + l.mv[k + 1],
                           (size_t)l.w[k + 1] * 2u, refineRadius, out, op);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace lfg
