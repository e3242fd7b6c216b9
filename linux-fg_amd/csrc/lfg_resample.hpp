// lfg_resample.hpp -- the tile plan and the two phase bodies of resample.hip (lfg_resample, include/linuxfg_hip.h) as
// __host__ __device__ functions of block index, thread index and an LDS pointer: the kernel calls them around its one
// barrier, and tests/cpp/resample_on_host.cpp, compiled with g++ alone, calls them from loops over blocks and threads --
// phase 1 for every thread of a block, then phase 2.  Nothing here needs the HIP runtime.
//
// A workgroup of kResampleThreads = 256 threads owns a tile of kResampleColumns = 64 output columns x T output rows.  The source
// rows that tile needs are rowLo = fy[q0] .. rowHi = fy[q1 - 1] + cy[q1 - 1] (first and first + count of a table do not
// decrease; resample_plan checks it anyway), at most kResampleLdsRows = 64 of them, and the horizontal pass of those rows
// lives in LDS only: one 8-byte word of four int16 per (source row, output column), consecutive columns at consecutive
// words, 32 KiB at the most.  The host picks T per call (resample_plan): the largest of 16, 8, 4, 2, 1 at which every tile's
// rows fit; one output row always does, a row having at most 64 taps.
//
//   phase 1   thread = (column c, row group g of 4).  A group takes the tile's source rows in blocks of kResampleBlock = 4
//             (block g, g + 4, ...): the taps of its column are count[p] consecutive dwords of a row from fx[p] on, taken
//             four at a time -- one 16-byte load from each of the four rows per 8-byte load of weights -- and the 1 .. 3
//             that remain one by one; neighbouring lanes read neighbouring or the same dwords.  h' goes to LDS as one 8-byte store.
//   barrier
//   phase 2   thread (c, g) forms output rows q0 + g, q0 + g + 4, ... of its column from the LDS column (the row, its first
//             tap and its weights are the same for a whole wave) and stores one dword per pixel: a wave stores 256 contiguous
//             bytes.
// The table guarantees first >= 0 and first + count <= in: no index is clamped here.  Byte offsets are size_t.
#pragma once

#include <cstddef>
#include <cstdint>

namespace lfg {

constexpr uint32_t kResampleColumns = 64;      // output columns of a tile = lanes of a wave
constexpr uint32_t kResampleGroups = 4;        // row groups = waves of a workgroup
constexpr uint32_t kResampleThreads = kResampleColumns * kResampleGroups;
constexpr uint32_t kResampleLdsRows = 64;      // source rows of a tile at the most (= LFG_RESAMPLE_MAX_TAPS)
constexpr uint32_t kResampleBlock = 4;         // source rows a thread takes per pass over its taps
constexpr uint32_t kResampleMaxRows = 16;      // the largest T

struct alignas(8) ResampleWord { uint32_t lo, hi; };          // h' of four channels: R | G << 16, B | A << 16

// One axis' table on the device: rows `stride` weights apart (the largest count rounded up to even, not 64).
struct ResampleAxis { const int32_t *first; const uint32_t *count; const int16_t *weights; uint32_t stride; };

struct ResampleArgs {
    const uint8_t *in; size_t inPitch;
    uint8_t *out; size_t outPitch;
    uint32_t outW, outH;
    ResampleAxis x, y;
    uint32_t rows;                             // T
};

struct ResamplePlan { uint32_t rows, span; };  // T, and the most source rows one of its tiles needs (LDS: span * 512 bytes)

// The plan of a vertical table (host only).
inline ResamplePlan resample_plan(const int32_t *first, const uint32_t *count, uint32_t outH) {
    for (uint32_t T = kResampleMaxRows; T > 1u; T /= 2u) {
        bool ok = true;
        uint32_t span = 0;
        for (uint32_t q0 = 0; q0 < outH && ok; q0 += (outH - q0 < T ? outH - q0 : T)) {
            const uint32_t q1 = outH - q0 < T ? outH : q0 + T;
            const int64_t lo = first[q0], hi = (int64_t)first[q1 - 1u] + (int64_t)count[q1 - 1u];
            for (uint32_t q = q0; q < q1; ++q) ok = ok && first[q] >= lo && (int64_t)first[q] + (int64_t)count[q] <= hi;
            ok = ok && hi - lo <= (int64_t)kResampleLdsRows;
            if (ok && (uint32_t)(hi - lo) > span) span = (uint32_t)(hi - lo);
        }
        if (ok) return ResamplePlan{T, span};
    }
    uint32_t span = 0;
    for (uint32_t q = 0; q < outH; ++q) span = count[q] > span ? count[q] : span;
    return ResamplePlan{1u, span};
}

// The tile (tileX, tileY): its output rows q0 .. q1 - 1 and its source rows rowLo .. rowHi - 1.
struct ResampleTile { uint32_t q0, q1; int32_t rowLo, rowHi; };

__host__ __device__ inline ResampleTile resample_tile(const ResampleArgs &a, uint32_t tileY) {
    ResampleTile t;
    t.q0 = tileY * a.rows;
    t.q1 = a.outH - t.q0 < a.rows ? a.outH : t.q0 + a.rows;
    t.rowLo = a.y.first[t.q0];
    t.rowHi = a.y.first[t.q1 - 1u] + (int32_t)a.y.count[t.q1 - 1u];
    return t;
}

// A value that has passed through here is not part of the shift-clamp-pack pattern that the compiler folds into an instruction
// the device gets wrong (yuv_convert.hip: kept_apart; the build's check_store_hazard.py refuses the instruction).
__host__ __device__ inline int resample_kept_apart(int v) {
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(v));
#endif
    return v;
}

__host__ __device__ inline int resample_byte(int v) {
    v = (v + (1 << 19)) >> 20;                                          // (arithmetic shift: floor)
    return resample_kept_apart(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Four consecutive texels / weights of a row, at the 4-byte alignment a texel and a table row have.
struct __attribute__((packed, aligned(4))) ResampleTexels4 { uint32_t t[4]; };
struct __attribute__((packed, aligned(4))) ResampleWeights4 { uint32_t w[2]; };

__host__ __device__ inline void resample_accumulate(int (&acc)[4], int w, uint32_t texel) {
    acc[0] += w * (int)(texel & 255u);
    acc[1] += w * (int)((texel >> 8) & 255u);
    acc[2] += w * (int)((texel >> 16) & 255u);
    acc[3] += w * (int)(texel >> 24);
}

// Phase 1 for thread (c, g) of tile (tileX, tileY): h' of column tileX * 64 + c for the source rows of the group's blocks.
__host__ __device__ inline void resample_phase1(const ResampleArgs &a, uint32_t tileX, uint32_t tileY, uint32_t c, uint32_t g,
                                                ResampleWord *lds) {
    const uint32_t p = tileX * kResampleColumns + c;
    if (p >= a.outW) return;
    const ResampleTile t = resample_tile(a, tileY);
    const size_t x0 = (size_t)a.x.first[p] * 4u;
    const uint32_t n = a.x.count[p];
    const int16_t *w = a.x.weights + (size_t)p * a.x.stride;
    for (int32_t r0 = t.rowLo + (int32_t)(g * kResampleBlock); r0 < t.rowHi; r0 += (int32_t)(kResampleGroups * kResampleBlock)) {
        // rows r0 .. r0 + 3; those past the tile's last row read that row again and are not written
        const uint8_t *row[kResampleBlock];
        int acc[kResampleBlock][4];
#pragma unroll
        for (uint32_t k = 0; k < kResampleBlock; ++k) {
            const int32_t r = r0 + (int32_t)k < t.rowHi ? r0 + (int32_t)k : t.rowHi - 1;
            row[k] = a.in + (size_t)r * a.inPitch + x0;
            acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
        }
        // four taps at a time through one 16-byte load per row and one 8-byte load of weights (both 4-byte aligned: a table
        // row starts at an even number of weights), then the 1 .. 3 taps that remain one by one
        uint32_t j = 0;
        for (; j + 4u <= n; j += 4u) {
            const ResampleWeights4 w4 = *reinterpret_cast<const ResampleWeights4 *>(w + j);
            const int wj[4] = {(int)(int16_t)(w4.w[0] & 0xffffu), (int)w4.w[0] >> 16, (int)(int16_t)(w4.w[1] & 0xffffu), (int)w4.w[1] >> 16};
#pragma unroll
            for (uint32_t k = 0; k < kResampleBlock; ++k) {
                const ResampleTexels4 t4 = *reinterpret_cast<const ResampleTexels4 *>(row[k] + (size_t)j * 4u);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) resample_accumulate(acc[k], wj[i], t4.t[i]);
            }
        }
        for (; j < n; ++j) {
            const int wj = w[j];
#pragma unroll
            for (uint32_t k = 0; k < kResampleBlock; ++k)
                resample_accumulate(acc[k], wj, *reinterpret_cast<const uint32_t *>(row[k] + (size_t)j * 4u));
        }
#pragma unroll
        for (uint32_t k = 0; k < kResampleBlock; ++k) {
            if (r0 + (int32_t)k >= t.rowHi) break;
            ResampleWord h;
            h.lo = ((uint32_t)((acc[k][0] + 128) >> 8) & 0xffffu) | ((uint32_t)((acc[k][1] + 128) >> 8) << 16);
            h.hi = ((uint32_t)((acc[k][2] + 128) >> 8) & 0xffffu) | ((uint32_t)((acc[k][3] + 128) >> 8) << 16);
            lds[(size_t)(r0 + (int32_t)k - t.rowLo) * kResampleColumns + c] = h;
        }
    }
}

// Phase 2 for thread (c, g): output rows q0 + g, q0 + g + 4, ... of column tileX * 64 + c.
__host__ __device__ inline void resample_phase2(const ResampleArgs &a, uint32_t tileX, uint32_t tileY, uint32_t c, uint32_t g,
                                                const ResampleWord *lds) {
    const uint32_t p = tileX * kResampleColumns + c;
    if (p >= a.outW) return;
    const ResampleTile t = resample_tile(a, tileY);
    for (uint32_t q = t.q0 + g; q < t.q1; q += kResampleGroups) {
        const uint32_t n = a.y.count[q];
        const int16_t *w = a.y.weights + (size_t)q * a.y.stride;
        const ResampleWord *col = lds + (size_t)(a.y.first[q] - t.rowLo) * kResampleColumns + c;
        int v[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < n; ++j) {
            const int wj = w[j];
            const ResampleWord h = col[(size_t)j * kResampleColumns];
            v[0] += wj * (int)(int16_t)(h.lo & 0xffffu);
            v[1] += wj * ((int)h.lo >> 16);
            v[2] += wj * (int)(int16_t)(h.hi & 0xffffu);
            v[3] += wj * ((int)h.hi >> 16);
        }
        const uint32_t px = (uint32_t)resample_byte(v[0]) | ((uint32_t)resample_byte(v[1]) << 8) | ((uint32_t)resample_byte(v[2]) << 16) |
                            ((uint32_t)resample_byte(v[3]) << 24);
        *reinterpret_cast<uint32_t *>(a.out + (size_t)q * a.outPitch + (size_t)p * 4u) = px;
    }
}

// ---- anti-ringing (lfg_resample_antiring, include/linuxfg_hip.h; resample_antiring.hip; tests/cpp/antiring_on_host.cpp)
//
// The same tile plan, LDS layout and thread roles as above; each phase additionally reads the two samples that bracket its
// output position on its axis -- a(p) <= b(p), both among the output's taps (lfg_resample_brackets) -- and pulls its sum
// towards their range by strength / 64.  A pass that is not anti-ringed has strength 0 and no bracket table: the mix is then
// the identity and the bracket is read at the first tap, so neither phase has a branch on the strength or on the content.
// Everything above stays as it is, loops included: resample_kernel's machine code is what section 4.16 measured.

struct ResampleBracket { const int32_t *lo, *hi; };           // a(p), b(p) of one growing axis on the device
struct ResampleAntiringArgs {
    ResampleArgs r;
    ResampleBracket bx, by;                    // of the width and of the height; not read where the strength is 0
    int sx, sy;                                // S where the horizontal / the vertical pass is anti-ringed, else 0
};

// What the sums can be.  A table row has sum q = 16384 and sum |q| <= 32768 (lfg_resample_taps refuses it otherwise), so its
// positive weights sum to at most 24576 and its negative ones to at least -8192:
//   h  in [-8192 * 255, 24576 * 255] = [-2,088,960, 6,266,880], and so is h clamped between two texels * 16384: |.| < 2^23;
//   h' in [-8160, 24480];  v in [-401,080,320, 668,467,200];  16384 h' in [-133,693,440, 401,080,320];
//   d = clamp(v) - v in [-802,160,640, 802,160,640]: |d| < 2^30.

// x * y for |x|, |y| < 2^23.  Saying that both are sign-extended from 24 bits is what lets the compiler take the full-rate
// 24-bit multiply (v_mul_i32_i24, v_mad_i32_i24), in which the two shifts disappear; the CPU computes the same number.
__host__ __device__ inline int resample_mul24(int x, int y) {
    return ((int)((uint32_t)x << 8) >> 8) * ((int)((uint32_t)y << 8) >> 8);
}

// The median of v, x and y: v clamped to the range of x and y, whichever of the two is the larger.  min(max(x, y), max(min(x, y), v))
// is the form the compiler turns into one v_med3_i32.
__host__ __device__ inline int resample_median(int v, int x, int y) {
    const int lo = x < y ? x : y, hi = x < y ? y : x, m = lo < v ? v : lo;
    return hi < m ? hi : m;
}

// The horizontal pass of one channel between the texels x and y, rounding included: with c = clamp(h, 16384 min, 16384 max),
// d = c - h and g = h + floor(d s / 64) = floor((64 h + d s) / 64), (g + 128) >> 8 = ((64 - s) h + s c + 8192) >> 14.
// Both products are 24-bit by the bounds above and their sum is 64 times a value between h and c.
// (x and y pass through resample_kept_apart so that the compiler forgets they are bytes: knowing it, it orders them with
// unsigned and h with signed minima and maxima, four instructions where the median is one.)
__host__ __device__ inline int resample_antiring_h(int h, int x, int y, int s) {
    const int c = resample_median(h, resample_kept_apart(x * 16384), resample_kept_apart(y * 16384));
    return (resample_mul24(64 - s, h) + resample_mul24(s, c) + 8192) >> 14;
}

// The vertical pass of one channel between the h' values x and y: v + floor(d s / 64) with d = clamp(v, 16384 min, 16384 max) - v.
// d s does not fit 32 bits; d = 256 (d >> 8) + (d & 255) gives floor(d s / 64) = 4 s (d >> 8) + ((d & 255) s >> 6), the same
// number as the 64-bit product's, from two 24-bit products (|d >> 8| < 2^22).  The result lies between v and the clamped v.
__host__ __device__ inline int resample_antiring_v(int v, int x, int y, int s) {
    const int d = resample_median(v, x * 16384, y * 16384) - v;
    return v + resample_mul24(d >> 8, 4 * s) + (resample_mul24(d & 255, s) >> 6);
}

// Phase 1 for thread (c, g), as resample_phase1: h' of its column for the source rows of the group's blocks, each sum mixed
// towards the range of the row's texels a(p) and b(p) before it is rounded.  The two texels are two more dword loads per row
// from cache lines that the taps bring in anyway (see the header of resample_antiring.hip).
__host__ __device__ inline void resample_antiring_phase1(const ResampleAntiringArgs &aa, uint32_t tileX, uint32_t tileY, uint32_t c,
                                                         uint32_t g, ResampleWord *lds) {
    const ResampleArgs &a = aa.r;
    const uint32_t p = tileX * kResampleColumns + c;
    if (p >= a.outW) return;
    const ResampleTile t = resample_tile(a, tileY);
    const size_t x0 = (size_t)a.x.first[p] * 4u;
    const size_t xa = aa.sx ? (size_t)aa.bx.lo[p] * 4u : x0, xb = aa.sx ? (size_t)aa.bx.hi[p] * 4u : x0;
    const uint32_t n = a.x.count[p];
    const int16_t *w = a.x.weights + (size_t)p * a.x.stride;
    for (int32_t r0 = t.rowLo + (int32_t)(g * kResampleBlock); r0 < t.rowHi; r0 += (int32_t)(kResampleGroups * kResampleBlock)) {
        const uint8_t *row[kResampleBlock];
        uint32_t ta[kResampleBlock], tb[kResampleBlock];
        int acc[kResampleBlock][4];
#pragma unroll
        for (uint32_t k = 0; k < kResampleBlock; ++k) {
            const int32_t r = r0 + (int32_t)k < t.rowHi ? r0 + (int32_t)k : t.rowHi - 1;
            row[k] = a.in + (size_t)r * a.inPitch;
            ta[k] = *reinterpret_cast<const uint32_t *>(row[k] + xa);
            tb[k] = *reinterpret_cast<const uint32_t *>(row[k] + xb);
            row[k] += x0;
            acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
        }
        uint32_t j = 0;
        for (; j + 4u <= n; j += 4u) {
            const ResampleWeights4 w4 = *reinterpret_cast<const ResampleWeights4 *>(w + j);
            const int wj[4] = {(int)(int16_t)(w4.w[0] & 0xffffu), (int)w4.w[0] >> 16, (int)(int16_t)(w4.w[1] & 0xffffu), (int)w4.w[1] >> 16};
#pragma unroll
            for (uint32_t k = 0; k < kResampleBlock; ++k) {
                const ResampleTexels4 t4 = *reinterpret_cast<const ResampleTexels4 *>(row[k] + (size_t)j * 4u);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) resample_accumulate(acc[k], wj[i], t4.t[i]);
            }
        }
        for (; j < n; ++j) {
            const int wj = w[j];
#pragma unroll
            for (uint32_t k = 0; k < kResampleBlock; ++k)
                resample_accumulate(acc[k], wj, *reinterpret_cast<const uint32_t *>(row[k] + (size_t)j * 4u));
        }
#pragma unroll
        for (uint32_t k = 0; k < kResampleBlock; ++k) {
            if (r0 + (int32_t)k >= t.rowHi) break;
            int h[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i)
                h[i] = resample_antiring_h(acc[k][i], (int)((ta[k] >> (8u * i)) & 255u), (int)((tb[k] >> (8u * i)) & 255u), aa.sx);
            ResampleWord word;
            word.lo = ((uint32_t)h[0] & 0xffffu) | ((uint32_t)h[1] << 16);
            word.hi = ((uint32_t)h[2] & 0xffffu) | ((uint32_t)h[3] << 16);
            lds[(size_t)(r0 + (int32_t)k - t.rowLo) * kResampleColumns + c] = word;
        }
    }
}

// Phase 2 for thread (c, g), as resample_phase2: each sum mixed towards the range of h' in the LDS rows a(q) and b(q) of its
// column -- two more 8-byte LDS reads per pixel, their rows the same for a whole wave like the taps'.
__host__ __device__ inline void resample_antiring_phase2(const ResampleAntiringArgs &aa, uint32_t tileX, uint32_t tileY, uint32_t c,
                                                         uint32_t g, const ResampleWord *lds) {
    const ResampleArgs &a = aa.r;
    const uint32_t p = tileX * kResampleColumns + c;
    if (p >= a.outW) return;
    const ResampleTile t = resample_tile(a, tileY);
    for (uint32_t q = t.q0 + g; q < t.q1; q += kResampleGroups) {
        const uint32_t n = a.y.count[q];
        const int16_t *w = a.y.weights + (size_t)q * a.y.stride;
        const int32_t first = a.y.first[q];
        const ResampleWord *col = lds + (size_t)(first - t.rowLo) * kResampleColumns + c;
        const ResampleWord ha = lds[(size_t)((aa.sy ? aa.by.lo[q] : first) - t.rowLo) * kResampleColumns + c];
        const ResampleWord hb = lds[(size_t)((aa.sy ? aa.by.hi[q] : first) - t.rowLo) * kResampleColumns + c];
        int v[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < n; ++j) {
            const int wj = w[j];
            const ResampleWord h = col[(size_t)j * kResampleColumns];
            v[0] += wj * (int)(int16_t)(h.lo & 0xffffu);
            v[1] += wj * ((int)h.lo >> 16);
            v[2] += wj * (int)(int16_t)(h.hi & 0xffffu);
            v[3] += wj * ((int)h.hi >> 16);
        }
        v[0] = resample_antiring_v(v[0], (int)(int16_t)(ha.lo & 0xffffu), (int)(int16_t)(hb.lo & 0xffffu), aa.sy);
        v[1] = resample_antiring_v(v[1], (int)ha.lo >> 16, (int)hb.lo >> 16, aa.sy);
        v[2] = resample_antiring_v(v[2], (int)(int16_t)(ha.hi & 0xffffu), (int)(int16_t)(hb.hi & 0xffffu), aa.sy);
        v[3] = resample_antiring_v(v[3], (int)ha.hi >> 16, (int)hb.hi >> 16, aa.sy);
        const uint32_t px = (uint32_t)resample_byte(v[0]) | ((uint32_t)resample_byte(v[1]) << 8) | ((uint32_t)resample_byte(v[2]) << 16) |
                            ((uint32_t)resample_byte(v[3]) << 24);
        *reinterpret_cast<uint32_t *>(a.out + (size_t)q * a.outPitch + (size_t)p * 4u) = px;
    }
}

// ---- linear and sigmoidal light (lfg_resample_light, include/linuxfg_hip.h; resample_light.hip; tests/cpp/light_on_host.cpp)
//
// The same tile plan, LDS row layout and thread roles as above.  The three colour bytes of a texel go through forward[256] into
// 14 bits of light before they are weighted and the sum goes back through threshold[255]; alpha keeps lfg_resample's formula.
// Both tables (lfg_light_tables) follow the tile's rows in LDS as uint16_t, forward then threshold, the 256th threshold slot
// holding 0xFFFF: kLightTableBytes behind span * 512 bytes of rows.  A workgroup stages them once (resample_light_stage), before
// its loop over tiles.  Everything above stays as it is: resample_kernel's machine code is what section 4.16 measured.
//
// What the sums can be, with forward in [0, 16383], sum q = 16384 and sum |q| <= 32768 of a table row:
//   h  = sum qx forward  in [-8192 * 16383, 24576 * 16383]: |h| < 2^29;
//   h' = (h + 8192) >> 14  in [-8192, 24575]: the int16 of the LDS word;
//   v  = sum qy h'  with |v| <= 32768 * 24575 < 2^31 - 8192;  L = clamp((v + 8192) >> 14, 0, 16383).

constexpr uint32_t kLightLevels = 256;                         // entries of each table in LDS
constexpr uint32_t kLightTableBytes = 2u * kLightLevels * sizeof(uint16_t);
constexpr int kLightOne = 16383;                               // forward[255]

struct ResampleLightArgs {
    ResampleArgs r;
    const uint32_t *tables;                    // forward[256] | threshold[255], 0xFFFF: 256 dwords on the device
    uint32_t span;                             // the plan's: the tables start span * 64 words into LDS
};

__host__ __device__ inline uint16_t *resample_light_tables(ResampleWord *lds, uint32_t span) {
    return reinterpret_cast<uint16_t *>(lds + (size_t)span * kResampleColumns);
}

// Staging for thread t of kResampleThreads = 256: one dword, two entries, of the 256 that both tables are.
__host__ __device__ inline void resample_light_stage(const ResampleLightArgs &la, uint32_t t, ResampleWord *lds) {
    reinterpret_cast<uint32_t *>(resample_light_tables(lds, la.span))[t] = la.tables[t];
}

__host__ __device__ inline void resample_light_accumulate(int (&acc)[4], int w, uint32_t texel, const uint16_t *forward) {
    acc[0] += w * (int)forward[texel & 255u];
    acc[1] += w * (int)forward[(texel >> 8) & 255u];
    acc[2] += w * (int)forward[(texel >> 16) & 255u];
    acc[3] += w * (int)(texel >> 24);
}

// to_byte: the number of thresholds <= L, found in eight steps without a branch.  Step s reads threshold[pos + s - 1] with pos a
// multiple of 2 s that is at most 256 - 2 s: index 254 at the most.
__host__ __device__ inline int resample_light_byte(int v, const uint16_t *threshold) {
    int L = (v + 8192) >> 14;                                           // (arithmetic shift: floor)
    L = L < 0 ? 0 : L > kLightOne ? kLightOne : L;
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = kLightLevels / 2u; s > 0u; s /= 2u) pos += (int)threshold[pos + s - 1u] <= L ? s : 0u;
    return (int)pos;
}

// Phase 1 for thread (c, g), as resample_phase1: h' of its column for the source rows of the group's blocks, the colour bytes
// looked up in forward[] per tap.
__host__ __device__ inline void resample_light_phase1(const ResampleLightArgs &la, uint32_t tileX, uint32_t tileY, uint32_t c, uint32_t g,
                                                      ResampleWord *lds) {
    const ResampleArgs &a = la.r;
    const uint32_t p = tileX * kResampleColumns + c;
    if (p >= a.outW) return;
    const uint16_t *forward = resample_light_tables(lds, la.span);
    const ResampleTile t = resample_tile(a, tileY);
    const size_t x0 = (size_t)a.x.first[p] * 4u;
    const uint32_t n = a.x.count[p];
    const int16_t *w = a.x.weights + (size_t)p * a.x.stride;
    for (int32_t r0 = t.rowLo + (int32_t)(g * kResampleBlock); r0 < t.rowHi; r0 += (int32_t)(kResampleGroups * kResampleBlock)) {
        const uint8_t *row[kResampleBlock];
        int acc[kResampleBlock][4];
#pragma unroll
        for (uint32_t k = 0; k < kResampleBlock; ++k) {
            const int32_t r = r0 + (int32_t)k < t.rowHi ? r0 + (int32_t)k : t.rowHi - 1;
            row[k] = a.in + (size_t)r * a.inPitch + x0;
            acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
        }
        uint32_t j = 0;
        for (; j + 4u <= n; j += 4u) {
            const ResampleWeights4 w4 = *reinterpret_cast<const ResampleWeights4 *>(w + j);
            const int wj[4] = {(int)(int16_t)(w4.w[0] & 0xffffu), (int)w4.w[0] >> 16, (int)(int16_t)(w4.w[1] & 0xffffu), (int)w4.w[1] >> 16};
#pragma unroll
            for (uint32_t k = 0; k < kResampleBlock; ++k) {
                const ResampleTexels4 t4 = *reinterpret_cast<const ResampleTexels4 *>(row[k] + (size_t)j * 4u);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) resample_light_accumulate(acc[k], wj[i], t4.t[i], forward);
            }
        }
        for (; j < n; ++j) {
            const int wj = w[j];
#pragma unroll
            for (uint32_t k = 0; k < kResampleBlock; ++k)
                resample_light_accumulate(acc[k], wj, *reinterpret_cast<const uint32_t *>(row[k] + (size_t)j * 4u), forward);
        }
#pragma unroll
        for (uint32_t k = 0; k < kResampleBlock; ++k) {
            if (r0 + (int32_t)k >= t.rowHi) break;
            ResampleWord h;
            h.lo = ((uint32_t)((acc[k][0] + 8192) >> 14) & 0xffffu) | ((uint32_t)((acc[k][1] + 8192) >> 14) << 16);
            h.hi = ((uint32_t)((acc[k][2] + 8192) >> 14) & 0xffffu) | ((uint32_t)((acc[k][3] + 128) >> 8) << 16);
            lds[(size_t)(r0 + (int32_t)k - t.rowLo) * kResampleColumns + c] = h;
        }
    }
}

// Phase 2 for thread (c, g), as resample_phase2: the three colour sums go back to bytes through threshold[], alpha through
// resample_byte.
__host__ __device__ inline void resample_light_phase2(const ResampleLightArgs &la, uint32_t tileX, uint32_t tileY, uint32_t c, uint32_t g,
                                                      const ResampleWord *lds) {
    const ResampleArgs &a = la.r;
    const uint32_t p = tileX * kResampleColumns + c;
    if (p >= a.outW) return;
    const uint16_t *threshold = reinterpret_cast<const uint16_t *>(lds + (size_t)la.span * kResampleColumns) + kLightLevels;
    const ResampleTile t = resample_tile(a, tileY);
    for (uint32_t q = t.q0 + g; q < t.q1; q += kResampleGroups) {
        const uint32_t n = a.y.count[q];
        const int16_t *w = a.y.weights + (size_t)q * a.y.stride;
        const ResampleWord *col = lds + (size_t)(a.y.first[q] - t.rowLo) * kResampleColumns + c;
        int v[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < n; ++j) {
            const int wj = w[j];
            const ResampleWord h = col[(size_t)j * kResampleColumns];
            v[0] += wj * (int)(int16_t)(h.lo & 0xffffu);
            v[1] += wj * ((int)h.lo >> 16);
            v[2] += wj * (int)(int16_t)(h.hi & 0xffffu);
            v[3] += wj * ((int)h.hi >> 16);
        }
        const uint32_t px = (uint32_t)resample_light_byte(v[0], threshold) | ((uint32_t)resample_light_byte(v[1], threshold) << 8) |
                            ((uint32_t)resample_light_byte(v[2], threshold) << 16) | ((uint32_t)resample_byte(v[3]) << 24);
        *reinterpret_cast<uint32_t *>(a.out + (size_t)q * a.outPitch + (size_t)p * 4u) = px;
    }
}

}  // namespace lfg
