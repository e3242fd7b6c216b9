// frame_diff.hip -- exact integer comparison of two RGBA8 frames (lfg_frame_diff, include/linuxfg_hip.h).  No reference
// counterpart; opt-in, outside the three stages.  tests/diff_model.py restates the definition on the CPU.
//
// frame_diff_kernel  per pixel the four absolute byte differences d_c, their squares summed per channel, and a histogram of
//                    m = the largest d_c over the channels of the mask.  8 bytes read per pixel, nothing written but the record.
//
// A record kernel: the fixed grid, the walk's cursor, the division by a multiplier and the refusals are lfg_record_plan.hpp's,
// the wave sums, the workgroup's merge and the LDS bins' one-lane add lfg_record.hpp's.  What is this file's:
//   * An item of the walk is four pixels of one row through one 16-byte load per frame (kWide), or one pixel through a dword
//     load, as lfg_record_plan.hpp splits the width (launch_frame_diff: two launches onto one record).  The cursor is (row,
//     item of the row), per lane; the byte offsets of both frames ride along with it and wrap where it wraps.  Every lane
//     runs the same number of trips, kDiffUnroll items per trip, so that the ballots below see the whole wave; an item past
//     the end loads from (0, 0) and counts nowhere.
//   * Squares: d_c^2 <= 65,025, so the at most kDiffUnroll * 4 = 8 pixels of ONE trip sum to at most 520,200 per channel in
//     32 bits; each trip ends by adding these four partials into four 64-bit registers (flush every trip: 8 adds per 8
//     pixels instead of a quarter-rate 64-bit multiply-add per channel and pixel).
//   * The histogram: bins 0 and 1 are counted by ballot + population count into a wave-uniform 64-bit scalar -- two frames
//     that are nearly the same put every pixel there, and 64 lanes adding to one LDS word serialise.  Only the pixels with
//     m >= 2 go to the LDS bins; where no lane has such a pixel the wave skips all of that.
// No float anywhere.  All 261 results are integers: neither the walk nor the order of the atomics changes them.
//
// Traffic per pixel: 4 (a) + 4 (b) = 8 bytes, 66.4 MB at 4K.
#include "lfg_internal.hpp"
#include "lfg_record.hpp"
#include "lfg_record_plan.hpp"

namespace lfg {
namespace {

constexpr int kDiffThreads = 1024;                          // 16 waves: one LDS histogram and one merge for all of them
constexpr int kDiffWaves = kDiffThreads / 64;
constexpr int kDiffGroupsPerCu = 2;                         // workgroups per CU of the fixed grid
constexpr int kDiffUnroll = 2;                              // items per trip of the walk
constexpr int kDiffBins = 256;
// The most pixels one workgroup may see in a launch (launch_frame_diff sizes the grid by it): what keeps a 32-bit LDS bin exact.
constexpr unsigned long long kDiffGroupPixels = 1ull << 31;

// The texels of an item of both frames, at byte offsets aOff / bOff.  The loads are unconditional: where there is no item
// they come from the frames' first bytes, and the caller leaves them out.
template <bool kWide>
__device__ __forceinline__ void diff_loads(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, bool item, size_t aOff,
                                           size_t bOff, uint32_t (&pa)[4], uint32_t (&pb)[4]) {
    const uint8_t *__restrict__ ta = a + (item ? aOff : (size_t)0);
    const uint8_t *__restrict__ tb = b + (item ? bOff : (size_t)0);
    if (kWide) {
        const uint4 va = *reinterpret_cast<const uint4 *>(ta);
        const uint4 vb = *reinterpret_cast<const uint4 *>(tb);
        pa[0] = va.x; pa[1] = va.y; pa[2] = va.z; pa[3] = va.w;
        pb[0] = vb.x; pb[1] = vb.y; pb[2] = vb.z; pb[3] = vb.w;
    } else {
        pa[0] = *reinterpret_cast<const uint32_t *>(ta);
        pb[0] = *reinterpret_cast<const uint32_t *>(tb);
    }
}

template <bool kWide>
__global__ __launch_bounds__(kDiffThreads) void frame_diff_kernel(
        const uint8_t *__restrict__ a, size_t aPitch, const uint8_t *__restrict__ b, size_t bPitch, uint32_t H,
        uint32_t itemsX, unsigned long long divMagic, uint32_t divShift, uint32_t stepRow, uint32_t stepG, uint32_t trips,
        uint32_t channelMask, unsigned long long pixels, unsigned long long *__restrict__ stats) {
    constexpr int kPixels = kWide ? 4 : 1;
    constexpr size_t kItemBytes = 4u * kPixels;
    // 32 bits per bin: a workgroup sees at most kDiffGroupPixels = 2^31 pixels in a launch (launch_frame_diff), bins 0 and 1
    // of this array are never used, and the bins are merged once, at the end.
    __shared__ uint32_t bins[kDiffBins];
    __shared__ unsigned long long part[6][kDiffWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < (uint32_t)kDiffBins) bins[tid] = 0u;
    __syncthreads();

    uint32_t keep[4];                                        // all ones for a channel of the mask
#pragma unroll
    for (int c = 0; c < 4; ++c) keep[c] = (channelMask >> c) & 1u ? 0xffffffffu : 0u;

    // this lane's first item as (row, item of the row), and the step between its items in bytes of either frame
    RecordCursor<unsigned long long> at = record_cursor<unsigned long long>(blockIdx.x * (uint32_t)kDiffThreads + tid, itemsX, divMagic, divShift);
    size_t aOff = (size_t)at.major * aPitch + (size_t)at.minor * kItemBytes, bOff = (size_t)at.major * bPitch + (size_t)at.minor * kItemBytes;
    const size_t aStep = (size_t)stepRow * aPitch + (size_t)stepG * kItemBytes, bStep = (size_t)stepRow * bPitch + (size_t)stepG * kItemBytes;
    const size_t aWrap = aPitch - (size_t)itemsX * kItemBytes, bWrap = bPitch - (size_t)itemsX * kItemBytes;      // modulo 2^64

    unsigned long long sse[4] = {0ull, 0ull, 0ull, 0ull};    // this lane's pixels
    unsigned long long zeros = 0ull, ones = 0ull;            // this wave's pixels with m = 0, m = 1 (wave-uniform)
    for (uint32_t t = 0; t < trips; ++t) {
        uint32_t pa[kDiffUnroll][4], pb[kDiffUnroll][4];
        bool item[kDiffUnroll];
#pragma unroll
        for (int k = 0; k < kDiffUnroll; ++k) {
            item[k] = at.major < (unsigned long long)H;
            diff_loads<kWide>(a, b, item[k], aOff, bOff, pa[k], pb[k]);
            aOff += aStep;
            bOff += bStep;
            at.advance(stepRow, stepG, itemsX, [&] { aOff += aWrap; bOff += bWrap; });
        }
        uint32_t sq[4] = {0u, 0u, 0u, 0u};                   // one trip's squares: at most 8 * 65,025
#pragma unroll
        for (int k = 0; k < kDiffUnroll; ++k) {
#pragma unroll
            for (int i = 0; i < kPixels; ++i) {
                const bool pixel = item[k];
                const uint32_t u = pa[k][i], v = pixel ? pb[k][i] : u;
                uint32_t m = 0u;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t byte = 0xffu << (8 * c);
                    const uint32_t d = __builtin_amdgcn_sad_u8(u & byte, v & byte, 0u);      // |a_c - b_c|: the other bytes are 0
                    sq[c] += __umul24(d, d);
                    m = max(m, d & keep[c]);
                }
                zeros += (unsigned long long)__popcll(__ballot(pixel && m == 0u));
                ones += (unsigned long long)__popcll(__ballot(pixel && m == 1u));
                const unsigned long long rest = __ballot(pixel && m >= 2u);
                if (rest != 0ull) bins_add(bins, m, pixel, pixel && m >= 2u, rest, lane);      // wave-uniform
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sse[c] += sq[c];
    }

#pragma unroll
    for (int c = 0; c < 4; ++c) sse[c] = wave_sum_u64(sse[c]);
    if (lane == 0u) {
        const uint32_t w = tid >> 6;
#pragma unroll
        for (int c = 0; c < 4; ++c) part[c][w] = sse[c];
        part[4][w] = zeros;
        part[5][w] = ones;
    }
    __syncthreads();
    // the record: pixels, sse[4], hist[256]
    if (tid < 6u) {
        record_add(stats + 1 + tid, group_sum_u64(part[tid]));                     // sse[0..3], then hist[0] and hist[1]: words 1 .. 6
    } else if (tid == 6u) {
        if (blockIdx.x == 0) atomicAdd(stats, pixels);       // onto the cleared word, or onto the record's own count
    }
    if (tid >= 2u && tid < (uint32_t)kDiffBins) {
        record_add(stats + 5 + tid, bins[tid]);
    }
}

// One launch over the W x H pixels at a / b.
hipError_t launch_diff_part(hipStream_t s, bool wide, const uint8_t *a, size_t aPitch, const uint8_t *b, size_t bPitch, uint32_t W,
                            uint32_t H, uint32_t channelMask, int deviceCus, unsigned long long *stats) {
    const uint32_t itemsX = wide ? W / 4u : W;
    RecordGrid g;                                            // an item is at most 4 pixels
    if (!record_fixed_grid<unsigned long long>(itemsX, H, kDiffThreads, kDiffUnroll, kDiffGroupsPerCu, deviceCus, kDiffGroupPixels / 4ull, g))
        return hipErrorInvalidValue;
    const RecordDivisor d = record_divisor(itemsX);
    const auto kernel = wide ? frame_diff_kernel<true> : frame_diff_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(kDiffThreads), 0, s, a, aPitch, b, bPitch, H, itemsX, d.magic, d.shift,
                       (uint32_t)(g.stride / itemsX), (uint32_t)(g.stride % itemsX), g.trips, channelMask, (unsigned long long)W * H, stats);
    return hipGetLastError();
}

}  // namespace

// The clear, then the parts of the width, both adding to the record (each its own share of `pixels`).
hipError_t launch_frame_diff(hipStream_t s, const lfg_frame &a, const lfg_frame &b, uint32_t channelMask, bool accumulate,
                             int deviceCus, void *stats) {
    const uint8_t *pa = (const uint8_t *)a.data, *pb = (const uint8_t *)b.data;
    const uint32_t W = a.width, H = a.height;
    const uint32_t wideW = wide_columns(multiples_of_16(a.data, b.data, a.pitch, b.pitch), W);
    hipError_t e = record_clear(s, stats, sizeof(lfg_frame_diff_stats), accumulate);
    if (e != hipSuccess) return e;
    if (wideW != 0u) {
        e = launch_diff_part(s, true, pa, a.pitch, pb, b.pitch, wideW, H, channelMask, deviceCus, (unsigned long long *)stats);
        if (e != hipSuccess) return e;
    }
    if (wideW == W) return hipSuccess;
    return launch_diff_part(s, false, pa + (size_t)wideW * 4u, a.pitch, pb + (size_t)wideW * 4u, b.pitch, W - wideW, H, channelMask,
                            deviceCus, (unsigned long long *)stats);
}

}  // namespace lfg
