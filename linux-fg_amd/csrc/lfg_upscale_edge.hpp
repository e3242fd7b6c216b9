// lfg_upscale_edge.hpp -- the tile and the two phase bodies of upscale_edge.hip (lfg_upscale_edge, include/linuxfg_hip.h, which
// has the definition) as __host__ __device__ functions of tile index, thread index and an LDS pointer, as lfg_resample.hpp has
// resample.hip's: the kernel calls them around its one barrier, and tests/cpp/upscale_edge_on_host.cpp, compiled with g++
// alone, calls them from loops over tiles and threads.  Nothing here needs the HIP runtime.
//
// A workgroup of kEdgeThreads = 256 threads owns a tile of kEdgeColumns = 64 x kEdgeRows = 16 output pixels.  The base of an
// axis does not decrease and grows by at most 1 per output sample (out >= in; the host checks its table), so the brackets of
// a tile lie in X0 = base[first column] .. X1 + 1 with X1 = base[last column] <= X0 + 63, and likewise in Y0 .. Y1 + 1:
//
//   phase 1   the texels (X0 - 1 .. X1 + 2) x (Y0 - 1 .. Y1 + 2), every coordinate clamped to the frame, go to LDS as dwords --
//             at most 67 x 19 -- and the analysis (dX, dY, mX, mY) of the texels (X0 .. X1 + 1) x (Y0 .. Y1 + 1), at most 65 x 17,
//             as one 8-byte word each: computed once per texel from five dword loads (the texel and its four clamped
//             neighbours; lines the staging of the same wave fetches anyway).  Thread (c, g) takes rows g, g + 4, ... and in
//             each the columns c and, where the row is longer than 64, c + 64.
//   barrier
//   phase 2   thread (c, g) forms output rows q0 + g, q0 + g + 4, ... of column tileX * 64 + c: four analysis words, the shape
//             row (16 bytes from global memory through the cache: 528 rows, 8.25 KiB), twelve texels from LDS, the weights, one
//             reciprocal and four exact quotients, one dword store -- a wave stores 256 contiguous bytes.
// Every product is between numbers below 2^23 in magnitude (the bounds stand at each), said through resample_mul24 so that the
// compiler takes the full-rate 24-bit multiply.  Byte offsets are size_t.
#pragma once

#include <cstddef>
#include <cstdint>

#include "lfg_resample.hpp"

namespace lfg {

constexpr uint32_t kEdgeColumns = 64;          // output columns of a tile = lanes of a wave
constexpr uint32_t kEdgeRows = 16;             // output rows of a tile
constexpr uint32_t kEdgeGroups = 4;            // row groups = waves of a workgroup
constexpr uint32_t kEdgeThreads = kEdgeColumns * kEdgeGroups;
constexpr uint32_t kEdgeTexW = kEdgeColumns + 3, kEdgeTexH = kEdgeRows + 3;      // staged texels of a tile at the most
constexpr uint32_t kEdgeAnaW = kEdgeColumns + 1, kEdgeAnaH = kEdgeRows + 1;      // analysed texels of a tile at the most
constexpr int kEdgeDirections = 16, kEdgeStrengths = 33;
constexpr int kEdgeFlat = 4 * 65536;

struct alignas(8) EdgeAnalysis { uint32_t d, m; };            // dX | dY << 16 (both signed), mX | mY << 16
struct alignas(16) EdgeShape { int16_t A, B, C, lob, clp, unused[3]; };   // a row of lfg_upscale_edge_shapes on the device
struct EdgeAxis { const int32_t *base; const uint8_t *frac; };             // lfg_upscale_edge_positions of one axis on the device

struct EdgeLds {
    uint32_t tex[kEdgeTexH][kEdgeTexW];
    EdgeAnalysis ana[kEdgeAnaH][kEdgeAnaW];
};

struct EdgeArgs {
    const uint8_t *in; size_t inPitch;
    uint8_t *out; size_t outPitch;
    uint32_t inW, inH, outW, outH;
    EdgeAxis x, y;
    const EdgeShape *shapes;                   // [k * 33 + q]
};

// The tile (tileX, tileY): its output columns p0 .. p1 - 1 and rows q0 .. q1 - 1, and the bases of its first and last ones.
struct EdgeTile { uint32_t p0, p1, q0, q1; int32_t X0, X1, Y0, Y1; };

__host__ __device__ inline EdgeTile edge_tile(const EdgeArgs &a, uint32_t tileX, uint32_t tileY) {
    EdgeTile t;
    t.p0 = tileX * kEdgeColumns;
    t.p1 = a.outW - t.p0 < kEdgeColumns ? a.outW : t.p0 + kEdgeColumns;
    t.q0 = tileY * kEdgeRows;
    t.q1 = a.outH - t.q0 < kEdgeRows ? a.outH : t.q0 + kEdgeRows;
    t.X0 = a.x.base[t.p0]; t.X1 = a.x.base[t.p1 - 1u];
    t.Y0 = a.y.base[t.q0]; t.Y1 = a.y.base[t.q1 - 1u];
    return t;
}

__host__ __device__ inline int edge_clamped(int v, int last) { return v < 0 ? 0 : v > last ? last : v; }
__host__ __device__ inline int edge_abs(int v) { return v < 0 ? -v : v; }
__host__ __device__ inline int edge_max(int a, int b) { return a > b ? a : b; }

// L = R + 2 G + B of a texel: 0 .. 1020.
__host__ __device__ inline int edge_luma(uint32_t t) { return (int)(t & 255u) + 2 * (int)((t >> 8) & 255u) + (int)((t >> 16) & 255u); }

// Phase 1 for thread (c, g) of tile (tileX, tileY).
__host__ __device__ inline void edge_phase1(const EdgeArgs &a, uint32_t tileX, uint32_t tileY, uint32_t c, uint32_t g, EdgeLds *lds) {
    const EdgeTile t = edge_tile(a, tileX, tileY);
    const int lastX = (int)a.inW - 1, lastY = (int)a.inH - 1;
    const uint32_t texW = (uint32_t)(t.X1 - t.X0) + 4u, texH = (uint32_t)(t.Y1 - t.Y0) + 4u;       // <= kEdgeTexW, kEdgeTexH
    for (uint32_t r = g; r < texH; r += kEdgeGroups) {
        const uint8_t *row = a.in + (size_t)edge_clamped(t.Y0 - 1 + (int)r, lastY) * a.inPitch;
        for (uint32_t col = c; col < texW; col += kEdgeColumns)
            lds->tex[r][col] = *reinterpret_cast<const uint32_t *>(row + (size_t)edge_clamped(t.X0 - 1 + (int)col, lastX) * 4u);
    }
    // the analysis of texel (X0 + col, Y0 + r) is that of the texel it clamps to, whose neighbours are clamped in their turn
    for (uint32_t r = g; r + 2u < texH; r += kEdgeGroups) {
        const int y = edge_clamped(t.Y0 + (int)r, lastY);
        const uint8_t *row = a.in + (size_t)y * a.inPitch;
        const uint8_t *up = a.in + (size_t)(y > 0 ? y - 1 : 0) * a.inPitch, *down = a.in + (size_t)(y < lastY ? y + 1 : lastY) * a.inPitch;
        for (uint32_t col = c; col + 2u < texW; col += kEdgeColumns) {
            const int x = edge_clamped(t.X0 + (int)col, lastX);
            const size_t at = (size_t)x * 4u, left = (size_t)(x > 0 ? x - 1 : 0) * 4u, right = (size_t)(x < lastX ? x + 1 : lastX) * 4u;
            const int m = edge_luma(*reinterpret_cast<const uint32_t *>(row + at));
            const int l = edge_luma(*reinterpret_cast<const uint32_t *>(row + left)), e = edge_luma(*reinterpret_cast<const uint32_t *>(row + right));
            const int u = edge_luma(*reinterpret_cast<const uint32_t *>(up + at)), d = edge_luma(*reinterpret_cast<const uint32_t *>(down + at));
            EdgeAnalysis w;
            w.d = ((uint32_t)(e - l) & 0xffffu) | ((uint32_t)(d - u) << 16);
            w.m = (uint32_t)edge_max(edge_abs(e - m), edge_abs(m - l)) | ((uint32_t)edge_max(edge_abs(d - m), edge_abs(m - u)) << 16);
            lds->ana[r][col] = w;
        }
    }
}

// Step 1: the smallest k that maximises |gx COS[k] + gy SIN[k]|; |gx|, |gy| <= 65,280 and the sum stays below 2^25.
__host__ __device__ inline int edge_direction(int gx, int gy) {
    constexpr int kCos[kEdgeDirections] = {256, 251, 237, 213, 181, 142, 98, 50, 0, -50, -98, -142, -181, -213, -237, -251};
    constexpr int kSin[kEdgeDirections] = {0, 50, 98, 142, 181, 213, 237, 251, 256, 251, 237, 213, 181, 142, 98, 50};
    int best = -1, k = 0;
#pragma unroll
    for (int n = 0; n < kEdgeDirections; ++n) {
        const int v = edge_abs(resample_mul24(gx, kCos[n]) + resample_mul24(gy, kSin[n]));
        k = v > best ? n : k;
        best = v > best ? v : best;
    }
    return k;
}

// Step 2: how many of M, 2 M, 3 M, 4 M are at most 4 A; 0 where M is 0.  A, M <= 65536 * 1020 < 2^26.
__host__ __device__ inline int edge_level(int A, int M) {
    const int a4 = 4 * A;
    return M == 0 ? 0 : (int)(a4 >= M) + (int)(a4 >= 2 * M) + (int)(a4 >= 3 * M) + (int)(a4 >= 4 * M);
}

// Step 5: the weight of the tap at (ox, oy) from the pixel, xx = (ox ox) >> 4 and yy = (oy oy) >> 4 given.  |ox|, |oy| <= 512:
// xx, yy, |(ox oy) >> 4| <= 16,384; A, C <= 2047, |B| <= 896; the sum stays below 2^27, d2 <= clp <= 19,508, |t1|, |t2| <= 4096.
__host__ __device__ inline int edge_weight(const EdgeShape &s, int ox, int oy, int xx, int yy) {
    const int sum = resample_mul24(s.A, xx) + resample_mul24(2 * s.B, resample_mul24(ox, oy) >> 4) + resample_mul24(s.C, yy);
    const int d2 = resample_median(sum >> 10, 0, s.clp);
    const int t1 = (resample_mul24(1638, d2) >> 12) - 4096, t2 = (resample_mul24(s.lob, d2) >> 12) - 4096;
    const int b = (resample_mul24(25, resample_mul24(t1, t1) >> 12) >> 4) - 2304;
    return resample_mul24(b, resample_mul24(t2, t2) >> 12) >> 12;
}

// floor(num / den) for 0 <= num < 2^26 and 0 < den < 2^15, rcp = 1 / den in float: the product is within 2^-21 of the
// quotient in relative terms and the quotient is below 2^14, so the estimate is off by one at the most, either way.
__host__ __device__ inline int edge_quotient(int num, int den, float rcp) {
    int q = (int)((float)num * rcp);
    const int r = num - resample_mul24(q, den);
    q = r < 0 ? q - 1 : q;
    return r >= den ? q + 1 : q;
}

// One output pixel: column and row of its bracket within the tile (ax = base - X0, ay = base - Y0) and its two fractions.
__host__ __device__ inline uint32_t edge_pixel(const EdgeLds *lds, const EdgeShape *shapes, int ax, int ay, int fx, int fy) {
    // the weighted sums over the bracket: w <= 65536 and the four sum to it
    int DX = 0, DY = 0, AX = 0, AY = 0, MX = 0, MY = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const EdgeAnalysis w = lds->ana[ay + j][ax + i];
            const int wt = (i ? fx : 256 - fx) * (j ? fy : 256 - fy);
            const int dX = (int)(int16_t)(w.d & 0xffffu), dY = (int)w.d >> 16;
            DX += resample_mul24(wt, dX); DY += resample_mul24(wt, dY);
            AX += resample_mul24(wt, edge_abs(dX)); AY += resample_mul24(wt, edge_abs(dY));
            MX += resample_mul24(wt, (int)(w.m & 0xffffu)); MY += resample_mul24(wt, (int)(w.m >> 16));
        }
    const bool flat = edge_max(edge_abs(DX), edge_abs(DY)) < kEdgeFlat;
    const int lx = edge_level(AX, MX), ly = edge_level(AY, MY);
    const int k = flat ? 0 : edge_direction(DX >> 10, DY >> 10), q = flat ? 0 : lx * lx + ly * ly;
    const EdgeShape s = shapes[k * kEdgeStrengths + q];

    int ox[4], oy[4], xx[4], yy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ox[i] = 256 * (i - 1) - fx; oy[i] = 256 * (i - 1) - fy;
        xx[i] = (ox[i] * ox[i]) >> 4; yy[i] = (oy[i] * oy[i]) >> 4;
    }
    int W = 0, S[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((i == 0 || i == 3) && (j == 0 || j == 3)) continue;
            const int wt = edge_weight(s, ox[i], oy[j], xx[i], yy[j]);
            const uint32_t texel = lds->tex[ay + j][ax + i];
            W += wt;
            resample_accumulate(S, wt, texel);                             // (|wt| <= 4096: 24-bit products)
        }
    // W is in 3364 .. 8356 whatever the shape and the fractions (tests/test_edge_model.py walks them all)
    const float rcp = 1.0f / (float)(2 * W);
    uint32_t px = 0u;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const uint32_t sh = 8u * (uint32_t)ch;
        const int b00 = (int)((lds->tex[ay + 1][ax + 1] >> sh) & 255u), b10 = (int)((lds->tex[ay + 1][ax + 2] >> sh) & 255u);
        const int b01 = (int)((lds->tex[ay + 2][ax + 1] >> sh) & 255u), b11 = (int)((lds->tex[ay + 2][ax + 2] >> sh) & 255u);
        const int lo = (b00 < b10 ? b00 : b10) < (b01 < b11 ? b01 : b11) ? (b00 < b10 ? b00 : b10) : (b01 < b11 ? b01 : b11);
        const int hi = edge_max(edge_max(b00, b10), edge_max(b01, b11));
        const int v = edge_quotient(edge_max(2 * S[ch] + W, 0), 2 * W, rcp);   // (a negative numerator ends at lo either way)
        px |= (uint32_t)resample_kept_apart(resample_median(v, lo, hi)) << sh;
    }
    return px;
}

// Phase 2 for thread (c, g): output rows q0 + g, q0 + g + 4, ... of column tileX * 64 + c.
__host__ __device__ inline void edge_phase2(const EdgeArgs &a, uint32_t tileX, uint32_t tileY, uint32_t c, uint32_t g, const EdgeLds *lds) {
    const EdgeTile t = edge_tile(a, tileX, tileY);
    const uint32_t p = t.p0 + c;
    if (p >= a.outW) return;
    const int ax = a.x.base[p] - t.X0, fx = a.x.frac[p];
    for (uint32_t q = t.q0 + g; q < t.q1; q += kEdgeGroups)
        *reinterpret_cast<uint32_t *>(a.out + (size_t)q * a.outPitch + (size_t)p * 4u) =
            edge_pixel(lds, a.shapes, ax, a.y.base[q] - t.Y0, fx, a.y.frac[q]);
}

}  // namespace lfg
