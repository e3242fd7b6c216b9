// frame_diff.hip -- exact integer comparison of two RGBA8 frames (lfg_frame_diff, include/linuxfg_hip.h).  No reference
// counterpart; opt-in, outside the three stages.  tests/diff_model.py restates the definition on the CPU.
//
// frame_diff_kernel  per pixel the four absolute byte differences d_c, their squares summed per channel, and a histogram of
//                    m = the largest d_c over the channels of the mask.  8 bytes read per pixel, nothing written but the record.
//
// The shape is pair_match_kernel's (pair_stats.hip): a FIXED grid of a few workgroups per CU, a grid-stride walk, 64-bit
// sums, one merge per workgroup, a clear of the record in front unless the call accumulates.  What differs:
//   * An item of the walk is four pixels of one row through one 16-byte load per frame (kWide), chosen by the host when the
//     base and the pitch of BOTH frames are multiples of 16; otherwise an item is one pixel through a dword load.  An item
//     is never partial: of a width that is no multiple of 4 the wide launch takes the columns up to the last multiple, and
//     a second, accumulating launch of the dword kernel the 1..3 columns that remain (launch_frame_diff).  Every lane runs
//     the same number of trips (the host's `trips`), kDiffUnroll items per trip, so that the ballots below see the whole
//     wave; an item past the end loads from (0, 0) and counts nowhere.
//   * Squares: d_c^2 <= 65,025, so the at most kDiffUnroll * 4 = 8 pixels of ONE trip sum to at most 520,200 per channel in
//     32 bits; each trip ends by adding these four partials into four 64-bit registers (flush every trip: 8 adds per 8
//     pixels instead of a quarter-rate 64-bit multiply-add per channel and pixel).
//   * The histogram: bins 0 and 1 are counted as pair_match_kernel counts its matches, ballot + population count into a
//     wave-uniform 64-bit scalar -- two frames that are nearly the same put every pixel there, and 64 lanes adding to one LDS
//     word serialise.  The pixels with m >= 2 go to a workgroup-private LDS histogram through ds_add_u32, unless all of them
//     in the wave share one m (0 against 255, a uniform offset): then one lane adds their number.  Where no lane has such a
//     pixel the wave skips all of that.
// No float anywhere.  All 261 results are integers: neither the walk nor the order of the atomics changes them.
//
// Traffic per pixel: 4 (a) + 4 (b) = 8 bytes, 66.4 MB at 4K.
#include <algorithm>

#include "lfg_internal.hpp"
#include "lfg_device.hpp"

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

    // this lane's first item, as (row, g): first / itemsX through the host's multiplier (launch_frame_diff: exact for
    // first < 2^31), not the compiler's division, which goes through a float reciprocal.  Then the step between its items:
    // gridDim.x * kDiffThreads of them, as rows and a rest, and the same in bytes of either frame.
    const uint32_t first = blockIdx.x * (uint32_t)kDiffThreads + tid;
    unsigned long long row = ((unsigned long long)first * divMagic) >> divShift;
    uint32_t g = first - (uint32_t)row * itemsX;
    size_t aOff = (size_t)row * aPitch + (size_t)g * kItemBytes, bOff = (size_t)row * bPitch + (size_t)g * kItemBytes;
    const size_t aStep = (size_t)stepRow * aPitch + (size_t)stepG * kItemBytes, bStep = (size_t)stepRow * bPitch + (size_t)stepG * kItemBytes;
    const size_t aWrap = aPitch - (size_t)itemsX * kItemBytes, bWrap = bPitch - (size_t)itemsX * kItemBytes;      // modulo 2^64

    unsigned long long sse[4] = {0ull, 0ull, 0ull, 0ull};    // this lane's pixels
    unsigned long long zeros = 0ull, ones = 0ull;            // this wave's pixels with m = 0, m = 1 (wave-uniform)
    for (uint32_t t = 0; t < trips; ++t) {
        uint32_t pa[kDiffUnroll][4], pb[kDiffUnroll][4];
        bool item[kDiffUnroll];
#pragma unroll
        for (int k = 0; k < kDiffUnroll; ++k) {
            item[k] = row < (unsigned long long)H;
            diff_loads<kWide>(a, b, item[k], aOff, bOff, pa[k], pb[k]);
            g += stepG;
            row += stepRow;
            aOff += aStep;
            bOff += bStep;
            if (g >= itemsX) { g -= itemsX; ++row; aOff += aWrap; bOff += bWrap; }
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
                if (rest != 0ull) {                          // wave-uniform
                    const int lead = __ffsll((long long)rest) - 1;
                    const uint32_t shared = (uint32_t)__builtin_amdgcn_readlane((int)m, lead);
                    if (__ballot(pixel && m == shared) == rest) {
                        if ((int)lane == lead) atomicAdd(&bins[shared], (uint32_t)__popcll(rest));
                    } else if (pixel && m >= 2u) {
                        atomicAdd(&bins[m], 1u);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) sse[c] += sq[c];
    }

#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sse[c] += __shfl_xor(sse[c], o, 64);
    if (lane == 0u) {
        const uint32_t w = tid >> 6;
#pragma unroll
        for (int c = 0; c < 4; ++c) part[c][w] = sse[c];
        part[4][w] = zeros;
        part[5][w] = ones;
    }
    __syncthreads();
    // the record: pixels, sse[4], hist[256].  Empty sums and bins add nothing; results unused: global_atomic_add_x2
    if (tid < 6u) {
        unsigned long long s = 0ull;
#pragma unroll
        for (int w = 0; w < kDiffWaves; ++w) s += part[tid][w];
        if (s != 0ull) atomicAdd(stats + 1 + tid, s);        // sse[0..3], then hist[0] and hist[1]: words 1 .. 6
    } else if (tid == 6u) {
        if (blockIdx.x == 0) atomicAdd(stats, pixels);       // onto the cleared word, or onto the record's own count
    }
    if (tid >= 2u && tid < (uint32_t)kDiffBins) {
        const uint32_t n = bins[tid];
        if (n != 0u) atomicAdd(stats + 5 + tid, (unsigned long long)n);
    }
}

}  // namespace

namespace {

// One launch over the W x H pixels at a / b.  Workgroups: kDiffGroupsPerCu per CU, never more than there are trips of work --
// and never so few that one of them would see more than kDiffGroupPixels pixels (a frame of that size does not fit a device
// of fewer CUs, but the 32-bit bins rest on it).
hipError_t launch_diff_part(hipStream_t s, bool wide, const uint8_t *a, size_t aPitch, const uint8_t *b, size_t bPitch, uint32_t W,
                            uint32_t H, uint32_t channelMask, int deviceCus, unsigned long long *stats) {
    const unsigned long long pixels = (unsigned long long)W * H;
    const uint32_t itemsX = wide ? W / 4u : W;
    const unsigned long long items = (unsigned long long)itemsX * H, perTrip = (unsigned long long)kDiffThreads * kDiffUnroll;
    // a workgroup takes at most items / grid + kDiffThreads * kDiffUnroll items (trips, rounded up), of at most 4 pixels each
    const unsigned long long atLeast = items / (kDiffGroupPixels / 4ull - perTrip) + 1ull;
    const unsigned long long fixed = (unsigned long long)std::max(deviceCus, 1) * kDiffGroupsPerCu;
    const unsigned long long grid = std::max(std::min((items + perTrip - 1) / perTrip, fixed), atLeast);
    const unsigned long long stride = grid * kDiffThreads;
    const unsigned long long trips = (items + stride * kDiffUnroll - 1) / (stride * kDiffUnroll);
    if (stride > 0x80000000ull || itemsX > 0x80000000u || trips > 0xffffffffull) return hipErrorInvalidValue;   // (no frame a device holds comes near)
    // n / itemsX for every n < 2^31 as (n * magic) >> shift: with 2^(l-1) < itemsX <= 2^l, magic = ceil(2^(31+l) / itemsX)
    // <= 2^32 and shift = 31 + l <= 63 (Granlund and Montgomery 1994, theorem 4.2); n * magic < 2^63
    uint32_t l = 0;
    while ((1ull << l) < (unsigned long long)itemsX) ++l;
    const uint32_t divShift = 31u + l;
    const unsigned long long divMagic = ((1ull << divShift) + itemsX - 1ull) / itemsX;
    const auto kernel = wide ? frame_diff_kernel<true> : frame_diff_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(kDiffThreads), 0, s, a, aPitch, b, bPitch, H, itemsX, divMagic, divShift,
                       (uint32_t)(stride / itemsX), (uint32_t)(stride % itemsX), (uint32_t)trips, channelMask, pixels, stats);
    return hipGetLastError();
}

}  // namespace

// The clear unless the call accumulates, then: the dword kernel over everything, or -- base and pitch of both frames multiples
// of 16 -- the 16-byte kernel over the columns up to the last multiple of 4 and the dword kernel over the 1..3 that remain,
// both adding to the record (each its own share of `pixels`).
hipError_t launch_frame_diff(hipStream_t s, const lfg_frame &a, const lfg_frame &b, uint32_t channelMask, bool accumulate,
                             int deviceCus, void *stats) {
    const uint8_t *pa = (const uint8_t *)a.data, *pb = (const uint8_t *)b.data;
    const uint32_t W = a.width, H = a.height;
    const bool wide = (((uintptr_t)a.data | (uintptr_t)b.data | (uintptr_t)a.pitch | (uintptr_t)b.pitch) % 16u) == 0 && W >= 4u;
    const uint32_t wideW = wide ? W & ~3u : 0u;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(stats, 0, sizeof(lfg_frame_diff_stats), s);
        if (e != hipSuccess) return e;
    }
    if (wideW != 0u) {
        hipError_t e = launch_diff_part(s, true, pa, a.pitch, pb, b.pitch, wideW, H, channelMask, deviceCus, (unsigned long long *)stats);
        if (e != hipSuccess) return e;
    }
    if (wideW == W) return hipSuccess;
    return launch_diff_part(s, false, pa + (size_t)wideW * 4u, a.pitch, pb + (size_t)wideW * 4u, b.pitch, W - wideW, H, channelMask,
                            deviceCus, (unsigned long long *)stats);
}

}  // namespace lfg
