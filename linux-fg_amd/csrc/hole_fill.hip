// hole_fill.hip -- the fill plane of the compensated family (lfg_hole_fill_plane, lfg_set_hole_reach, include/linuxfg_hip.h):
// for every pixel the order key that a hole there is filled with, from the nearest donor within `reach` in each of the four
// axis directions.  No reference counterpart; opt-in.  At reach 16 the plane holds at every hole what the walk of lfg_mc.hpp
// (mc_fill_vector) returns; its cost does not depend on how deep a hole is.  tests/fill_model.c restates the definition with
// plain loops.
//
// Two launches over the key image K, which neither of them writes:
//   fill_row_kernel  one wave per row, 256 pixels (four per lane) at a time from left to right.  "The nearest donor to the
//                    left" is a running maximum of (index, order key) and "to the right" a running minimum: inside a lane a
//                    loop over its four pixels, across the lanes one scan in the VALU (wave_scan), and from one 256-pixel
//                    segment to the next a carry in a register.  The reach is below a segment's width, so the minimum from
//                    the right needs the segment after the current one and nothing further; the loads run two segments ahead.
//                    Writes min(order(left), order(right)), the hole word where neither is within reach.
//   fill_col_kernel  one thread per column, 64 adjacent columns per wave (every row read is 256 contiguous bytes), one band of
//                    kFillBand rows per workgroup: a downward scan that starts `reach` rows above the band and an upward one
//                    that starts `reach` rows below it, both reading K alone, each folded into the thread's own word of the
//                    plane.  A band needs nothing from its neighbours.
// No atomics, and every trip count follows from the sizes, the reach and the band height alone.
//
// Traffic per pixel: the row pass reads K once and writes the plane once (8 bytes); the column pass reads K 2 (1 + reach /
// kFillBand) times and reads and writes the plane twice.
#include "lfg_mc.hpp"

namespace lfg {

namespace {

constexpr int kFillLanePixels = 4;
constexpr int kFillSegment = 64 * kFillLanePixels;         // pixels a wave scans at once
static_assert(kFillSegment > LFG_HOLE_REACH_MAX, "the row pass looks one segment ahead and no further");
constexpr int kFillRowWaves = 4;                           // rows per workgroup of the row pass
constexpr int kFillColBlock = 256;                         // columns per workgroup of the column pass

using u64 = unsigned long long;

template <bool PassStatic>
__device__ __forceinline__ bool fill_donor(uint32_t word) { return word != kMcHole && !(PassStatic && word == kMcStatic); }

// A donor as the scans carry it: its index (plus `bias`) above its order key.  Indices differ, so the largest value is the
// rightmost donor and the smallest the leftmost.
__device__ __forceinline__ u64 fill_pack(int index, uint32_t word) { return ((u64)(uint32_t)index << 32) | mv_key_flip_length(word); }

template <bool Suffix>
__device__ __forceinline__ u64 scan_op(u64 a, u64 b) { return Suffix ? (a < b ? a : b) : (a > b ? a : b); }

// One DPP move of a 64-bit value; lanes whose source does not exist get `identity`.
template <int Ctrl>
__device__ __forceinline__ u64 dpp_u64(u64 identity, u64 v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)identity, (int)(uint32_t)v, Ctrl, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(identity >> 32), (int)(uint32_t)(v >> 32), Ctrl, 0xF, 0xF, false);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 readlane_u64(u64 v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}

// The scan of one value per lane over the wave, every lane active.  Prefix: the maximum over the lanes below, identity 0.
// Suffix: the minimum over the lanes above, identity ~0.  `exclusive` leaves the lane's own value out, `total` is the whole
// wave's.  Four DPP steps inside each row of 16 lanes (row_shr / row_shl by 1, 2, 4, 8: max and min are idempotent, so the
// overlapping steps are harmless), the four rows' results through readlane, one wave shift for the exclusive form.
template <bool Suffix>
__device__ __forceinline__ void wave_scan(u64 v, int lane, u64 &exclusive, u64 &total) {
    constexpr u64 id = Suffix ? ~0ull : 0ull;
    constexpr int shift = Suffix ? 0x100 /* row_shl */ : 0x110 /* row_shr */;
    v = scan_op<Suffix>(v, dpp_u64<shift + 1>(id, v));
    v = scan_op<Suffix>(v, dpp_u64<shift + 2>(id, v));
    v = scan_op<Suffix>(v, dpp_u64<shift + 4>(id, v));
    v = scan_op<Suffix>(v, dpp_u64<shift + 8>(id, v));
    // the lane of each row that holds the row's result: its last (prefix) or its first (suffix)
    const u64 r0 = readlane_u64(v, Suffix ? 0 : 15), r1 = readlane_u64(v, Suffix ? 16 : 31);
    const u64 r2 = readlane_u64(v, Suffix ? 32 : 47), r3 = readlane_u64(v, Suffix ? 48 : 63);
    const int row = lane >> 4;
    u64 carry;
    if (Suffix) carry = row == 3 ? id : row == 2 ? r3 : row == 1 ? scan_op<true>(r2, r3) : scan_op<true>(r1, scan_op<true>(r2, r3));
    else carry = row == 0 ? id : row == 1 ? r0 : row == 2 ? scan_op<false>(r0, r1) : scan_op<false>(scan_op<false>(r0, r1), r2);
    v = scan_op<Suffix>(v, carry);
    total = scan_op<Suffix>(scan_op<Suffix>(r0, r1), scan_op<Suffix>(r2, r3));
    exclusive = dpp_u64<Suffix ? 0x130 /* wave_shl:1 */ : 0x138 /* wave_shr:1 */>(id, v);
}

struct FillWords { uint32_t w[kFillLanePixels]; };

// A lane's four words of a row from column x0 on, the hole word past the row's end: one 16-byte load where the row allows.
__device__ __forceinline__ FillWords fill_load(const uint32_t *__restrict__ row, bool aligned16, int x0, int W) {
    FillWords r;
    if (aligned16 && x0 + kFillLanePixels <= W) {
        const uint4 q = *reinterpret_cast<const uint4 *>(row + x0);
        r.w[0] = q.x; r.w[1] = q.y; r.w[2] = q.z; r.w[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kFillLanePixels; ++j) r.w[j] = x0 + j < W ? row[x0 + j] : kMcHole;
    }
    return r;
}

// The leftmost donor among a lane's four words (the value its lane brings to the suffix scan), ~0 if it has none.
template <bool PassStatic>
__device__ __forceinline__ u64 fill_first_donor(const FillWords &c, int x0) {
    u64 m = ~0ull;
#pragma unroll
    for (int j = kFillLanePixels - 1; j >= 0; --j)
        if (fill_donor<PassStatic>(c.w[j])) m = fill_pack(x0 + j, c.w[j]);
    return m;
}

// Pitches in words.  Block (64, kFillRowWaves): a wave is one row.
template <bool PassStatic>
__global__ __launch_bounds__(64 * kFillRowWaves) void fill_row_kernel(const uint32_t *__restrict__ keys, size_t keysPitch,
                                                                      uint32_t *__restrict__ plane, size_t planePitch, int W, int H,
                                                                      int reach) {
    const int lane = (int)threadIdx.x, y = (int)(blockIdx.x * kFillRowWaves + threadIdx.y);
    if (y >= H) return;                                            // the whole wave
    const uint32_t *__restrict__ row = keys + (size_t)y * keysPitch;
    uint32_t *__restrict__ dst = plane + (size_t)y * planePitch;
    const bool aligned16 = ((uintptr_t)row & 15u) == 0;
    const int lx = lane * kFillLanePixels;
    FillWords cur = fill_load(row, aligned16, lx, W), nxt = fill_load(row, aligned16, kFillSegment + lx, W);
    u64 carryLeft = 0, curRight, unusedTotal;                      // the rightmost donor of the segments behind: index + 1 above its key
    wave_scan<true>(fill_first_donor<PassStatic>(cur, lx), lane, curRight, unusedTotal);
    for (int seg = 0; seg < W; seg += kFillSegment) {
        const int x0 = seg + lx;
        const FillWords ahead = fill_load(row, aligned16, x0 + 2 * kFillSegment, W);
        u64 nxtRight, nxtFirst;
        wave_scan<true>(fill_first_donor<PassStatic>(nxt, x0 + kFillSegment), lane, nxtRight, nxtFirst);
        u64 mine = 0;                                              // the lane's rightmost donor
#pragma unroll
        for (int j = 0; j < kFillLanePixels; ++j)
            if (fill_donor<PassStatic>(cur.w[j])) mine = fill_pack(x0 + j + 1, cur.w[j]);
        u64 left, segLast;
        wave_scan<false>(mine, lane, left, segLast);
        left = scan_op<false>(left, carryLeft);
        u64 right = scan_op<true>(curRight, nxtFirst);
        uint32_t result[kFillLanePixels];
#pragma unroll
        for (int j = kFillLanePixels - 1; j >= 0; --j) {           // from the right: each pixel sees the donors after it
            result[j] = (uint32_t)(right >> 32) - (uint32_t)(x0 + j) <= (uint32_t)reach ? (uint32_t)right : kMcHole;   // none: index 2^32 - 1
            if (fill_donor<PassStatic>(cur.w[j])) right = fill_pack(x0 + j, cur.w[j]);
        }
#pragma unroll
        for (int j = 0; j < kFillLanePixels; ++j) {                // from the left: each pixel sees the donors before it
            const uint32_t at = (uint32_t)(left >> 32);            // index + 1, 0: none
            const uint32_t order = at != 0u && (uint32_t)(x0 + j + 1) - at <= (uint32_t)reach ? (uint32_t)left : kMcHole;
            result[j] = order < result[j] ? order : result[j];
            if (fill_donor<PassStatic>(cur.w[j])) left = fill_pack(x0 + j + 1, cur.w[j]);
        }
#pragma unroll
        for (int j = 0; j < kFillLanePixels; ++j)
            if (x0 + j < W) dst[x0 + j] = result[j];
        carryLeft = scan_op<false>(carryLeft, segLast);
        cur = nxt; curRight = nxtRight; nxt = ahead;
    }
}

// Pitches in words.  Block kFillColBlock: a thread is one column, a workgroup one band of `band` rows.
template <bool PassStatic>
__global__ __launch_bounds__(kFillColBlock) void fill_col_kernel(const uint32_t *__restrict__ keys, size_t keysPitch,
                                                                 uint32_t *__restrict__ plane, size_t planePitch, int W, int H, int reach,
                                                                 int band) {
    const int x = (int)(blockIdx.x * kFillColBlock + threadIdx.x);
    if (x >= W) return;
    const int y0 = (int)blockIdx.y * band, y1 = min(y0 + band, H);
    const uint32_t *__restrict__ k = keys + x;
    uint32_t *__restrict__ p = plane + x;
    int at = -2 * LFG_HOLE_REACH_MAX;                              // the row of the last donor seen; none yet: out of every reach
    uint32_t order = kMcHole;
#pragma unroll 8
    for (int y = max(y0 - reach, 0); y < y0; ++y) {                // downwards: the rows above the band
        const uint32_t word = k[(size_t)y * keysPitch];
        if (fill_donor<PassStatic>(word)) { at = y; order = mv_key_flip_length(word); }
    }
#pragma unroll 4
    for (int y = y0; y < y1; ++y) {
        const uint32_t word = k[(size_t)y * keysPitch], have = p[(size_t)y * planePitch];
        const uint32_t above = y - at <= reach ? order : kMcHole;
        p[(size_t)y * planePitch] = above < have ? above : have;
        if (fill_donor<PassStatic>(word)) { at = y; order = mv_key_flip_length(word); }
    }
    at = H + 2 * LFG_HOLE_REACH_MAX;
    order = kMcHole;
#pragma unroll 8
    for (int y = min(y1 - 1 + reach, H - 1); y >= y1; --y) {       // upwards: the rows below the band
        const uint32_t word = k[(size_t)y * keysPitch];
        if (fill_donor<PassStatic>(word)) { at = y; order = mv_key_flip_length(word); }
    }
#pragma unroll 4
    for (int y = y1 - 1; y >= y0; --y) {
        const uint32_t word = k[(size_t)y * keysPitch], have = p[(size_t)y * planePitch];
        const uint32_t below = at - y <= reach ? order : kMcHole;
        p[(size_t)y * planePitch] = below < have ? below : have;
        if (fill_donor<PassStatic>(word)) { at = y; order = mv_key_flip_length(word); }
    }
}

template <bool PassStatic>
hipError_t fill_launch(hipStream_t s, const uint32_t *keys, size_t keysPitch, uint32_t *plane, size_t planePitch, int W, int H,
                       int reach, int band) {
    hipLaunchKernelGGL(fill_row_kernel<PassStatic>, dim3((unsigned)((H + kFillRowWaves - 1) / kFillRowWaves)), dim3(64, kFillRowWaves),
                       0, s, keys, keysPitch, plane, planePitch, W, H, reach);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fill_col_kernel<PassStatic>, dim3((unsigned)((W + kFillColBlock - 1) / kFillColBlock), (unsigned)((H + band - 1) / band)),
                       dim3(kFillColBlock), 0, s, keys, keysPitch, plane, planePitch, W, H, reach, band);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_hole_fill_plane(hipStream_t s, const uint32_t *keys, size_t keysPitchWords, uint32_t *plane, size_t planePitchWords,
                                  int W, int H, int reach, bool passStatic, int band) {
    if (band <= 0) band = kFillBand;
    return passStatic ? fill_launch<true>(s, keys, keysPitchWords, plane, planePitchWords, W, H, reach, band)
                      : fill_launch<false>(s, keys, keysPitchWords, plane, planePitchWords, W, H, reach, band);
}

}  // namespace lfg
