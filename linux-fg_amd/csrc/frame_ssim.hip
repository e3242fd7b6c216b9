// frame_ssim.hip -- exact integer SSIM of two RGBA8 frames (lfg_frame_ssim, include/linuxfg_hip.h).  No reference counterpart;
// opt-in, outside the three stages.  tests/ssim_model.py restates the definition on the CPU.
//
// frame_ssim_kernel  per 8 x 8 window (2 x 2 blocks of 4 x 4 pixels, stride 4) and channel the sums s1, s2, ss, s12, from them
//                    Q_c = sign(N) floor(|N| 2^24 / D); the record takes the sum of Q_c per channel, a histogram of the smallest
//                    Q_c over the channels of the mask, and the smallest (value, wy, wx) key.  8 bytes read per pixel (plus one
//                    block row in kSsimSegmentRows and one block column in kSsimStripWindows read twice), nothing written but
//                    the record.
//
// The walk is per wave, with no LDS between a block and its window:
//   * A lane owns one 4 x 4 block: four rows of four texels per frame, through four 16-byte loads per frame (kWide), chosen by
//     the host when the base and the pitch of BOTH frames are multiples of 16, through sixteen dword loads otherwise.  Two
//     v_perm_b32 levels turn the four texels of a row into four channel dwords, and v_dot4_u32_u8 gives the row's share of
//     s1 (x . 0x01010101), s2, ss (x . x + y . y) and s12 (x . y).  A block's sums fit 32 bits (s <= 4,080: s1 and s2 share
//     one dword), a window's as well (s <= 16,320, ss <= 8,323,200, s12 <= 4,161,600).
//   * A wave owns kSsimStripWindows + 1 = 64 neighbouring blocks of a block row, so 63 windows: a lane adds the block of the
//     lane to its right (one cross-lane move per dword, twelve per block) and keeps that sum of two blocks for the block row
//     below, where the window is the kept sum plus the new one.  An item of the walk is a strip of 64 block columns by
//     kSsimSegmentRows window rows, so kSsimSegmentRows + 1 block rows; its first block row only fills the kept sums.  Lanes
//     past the last block column read the last one and their windows count nowhere.
//   * Items go to waves by lfg_record_plan.hpp's fixed grid and cursor, (segment, strip) per wave; every wave runs the host's
//     `trips`, and whether an item exists, how many block rows it has and which lanes hold a window follow from the sizes
//     alone.  The one data-dependent branch is wave-uniform: where N = D in every window of the wave (identical content:
//     Q = 2^24) the 25 steps of the restoring division are skipped for that channel.
//   * D < 2^58 and |N| <= D, so the division shifts a remainder below D left by one bit 24 times inside 64 bits.
//   * The histogram: bin 64 (identical windows) is counted by ballot and population count into a wave-uniform scalar -- two
//     frames that are the same put every window there; the other bins go to the workgroup's LDS bins.  The merge is
//     lfg_record.hpp's, with one 64-bit atomic minimum for the key beside the sums.
// No float anywhere.  All 71 results are integers: neither the walk nor the order of the atomics changes them.
#include "lfg_internal.hpp"
#include "lfg_record.hpp"
#include "lfg_record_plan.hpp"

namespace lfg {
namespace {

constexpr int kSsimWaves = 4;                               // waves per workgroup: one LDS histogram and one merge for them
constexpr int kSsimThreads = 64 * kSsimWaves;
constexpr int kSsimGroupsPerCu = 4;                         // workgroups per CU of the fixed grid
constexpr int kSsimStripWindows = 63;                       // windows of a block row that one wave owns: 64 blocks
constexpr int kSsimSegmentRows = 8;                         // window rows of an item: 9 block rows
constexpr int kSsimBins = 65;
constexpr int kSsimSums = 12;                               // per channel: s1 | s2 << 16, ss, s12
// The most windows one workgroup may see in a launch (launch_frame_ssim sizes the grid by it): what keeps a 32-bit LDS bin exact.
constexpr unsigned long long kSsimGroupWindows = 1ull << 31;
constexpr int32_t kSsimOne = 1 << 24;

// The four texels of a row as four dwords of one channel each (the order of the texels inside a dword is the same for both
// frames, which is all the dot products need).  v_perm_b32: selector bytes 0 .. 3 take from the second operand, 4 .. 7 from the first.
__device__ __forceinline__ void ssim_channels(const uint32_t (&p)[4], uint32_t (&ch)[4]) {
    const uint32_t rg01 = __builtin_amdgcn_perm(p[1], p[0], 0x05010400u), ba01 = __builtin_amdgcn_perm(p[1], p[0], 0x07030602u);
    const uint32_t rg23 = __builtin_amdgcn_perm(p[3], p[2], 0x05010400u), ba23 = __builtin_amdgcn_perm(p[3], p[2], 0x07030602u);
    ch[0] = __builtin_amdgcn_perm(rg23, rg01, 0x05040100u);
    ch[1] = __builtin_amdgcn_perm(rg23, rg01, 0x07060302u);
    ch[2] = __builtin_amdgcn_perm(ba23, ba01, 0x05040100u);
    ch[3] = __builtin_amdgcn_perm(ba23, ba01, 0x07060302u);
}

// The sums of the 4 x 4 block whose first texel is at byte offset aOff / bOff: out[3 c + 0 .. 2] = s1 | s2 << 16, ss, s12.
template <bool kWide>
__device__ __forceinline__ void ssim_block(const uint8_t *__restrict__ a, size_t aPitch, size_t aOff, const uint8_t *__restrict__ b,
                                           size_t bPitch, size_t bOff, uint32_t (&out)[kSsimSums]) {
    uint32_t pa[4][4], pb[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t *__restrict__ ta = a + aOff + (size_t)j * aPitch;
        const uint8_t *__restrict__ tb = b + bOff + (size_t)j * bPitch;
        if (kWide) {
            const uint4 va = *reinterpret_cast<const uint4 *>(ta);
            const uint4 vb = *reinterpret_cast<const uint4 *>(tb);
            pa[j][0] = va.x; pa[j][1] = va.y; pa[j][2] = va.z; pa[j][3] = va.w;
            pb[j][0] = vb.x; pb[j][1] = vb.y; pb[j][2] = vb.z; pb[j][3] = vb.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pa[j][i] = reinterpret_cast<const uint32_t *>(ta)[i];
                pb[j][i] = reinterpret_cast<const uint32_t *>(tb)[i];
            }
        }
    }
    uint32_t s1[4] = {0u, 0u, 0u, 0u}, s2[4] = {0u, 0u, 0u, 0u}, ss[4] = {0u, 0u, 0u, 0u}, s12[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t x[4], y[4];
        ssim_channels(pa[j], x);
        ssim_channels(pb[j], y);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s1[c] = __builtin_amdgcn_udot4(x[c], 0x01010101u, s1[c], false);
            s2[c] = __builtin_amdgcn_udot4(y[c], 0x01010101u, s2[c], false);
            ss[c] = __builtin_amdgcn_udot4(x[c], x[c], __builtin_amdgcn_udot4(y[c], y[c], ss[c], false), false);
            s12[c] = __builtin_amdgcn_udot4(x[c], y[c], s12[c], false);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        out[3 * c + 0] = s1[c] | (s2[c] << 16);
        out[3 * c + 1] = ss[c];
        out[3 * c + 2] = s12[c];
    }
}

// Q of one window and channel from its sums.  `live`: the lane holds a window (the others compute on repeated blocks and are
// left out by the caller).  Every operand fits: vars and the first factors below 2^31, covar inside int32, D < 2^58.
__device__ __forceinline__ int32_t ssim_q(uint32_t pk, uint32_t ss, uint32_t s12, bool live) {
    const uint32_t s1 = pk & 0xffffu, s2 = pk >> 16;
    const uint32_t cross = s1 * s2, squares = s1 * s1 + s2 * s2;
    const uint32_t vars = 64u * ss - squares;
    const int32_t covar = (int32_t)(64u * s12) - (int32_t)cross;
    const long long N = (long long)(int32_t)(2u * cross + 416u) * (long long)(2 * covar + 235963);
    const unsigned long long D = (unsigned long long)(squares + 416u) * (unsigned long long)(vars + 235963u);
    const unsigned long long mag = N < 0 ? (unsigned long long)-N : (unsigned long long)N;
    if (__ballot(live && mag != D) == 0ull) return kSsimOne;                     // wave-uniform: identical windows only
    // floor(mag 2^24 / D) with mag <= D < 2^58: bit 24 first, then 24 times a remainder below D doubled
    unsigned long long r = mag;
    uint32_t q = 0u;
#pragma unroll
    for (int i = 0; i < 25; ++i) {
        if (i > 0) r <<= 1;
        q <<= 1;
        if (r >= D) { r -= D; q |= 1u; }
    }
    return N < 0 ? -(int32_t)q : (int32_t)q;
}

template <bool kWide>
__global__ __launch_bounds__(kSsimThreads) void frame_ssim_kernel(
        const uint8_t *__restrict__ a, size_t aPitch, const uint8_t *__restrict__ b, size_t bPitch, uint32_t bw, uint32_t bh,
        uint32_t strips, uint32_t segments, unsigned long long divMagic, uint32_t divShift, uint32_t stepSegment, uint32_t stepStrip,
        uint32_t trips, uint32_t channelMask, unsigned long long windows, unsigned long long *__restrict__ stats) {
    // 32 bits per bin: a workgroup sees at most kSsimGroupWindows = 2^31 windows in a launch (launch_frame_ssim)
    __shared__ uint32_t bins[kSsimBins];
    __shared__ unsigned long long part[5][kSsimWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    if (tid < (uint32_t)kSsimBins) bins[tid] = 0u;
    __syncthreads();

    RecordCursor<uint32_t> at = record_cursor<uint32_t>(blockIdx.x * (uint32_t)kSsimWaves + wave, strips, divMagic, divShift);      // (segment, strip)

    unsigned long long sum[4] = {0ull, 0ull, 0ull, 0ull};    // this lane's windows, two's complement
    unsigned long long best = ~0ull;                         // this lane's smallest key
    uint32_t identical = 0u;                                 // this wave's windows in bin 64 (wave-uniform)
    for (uint32_t t = 0; t < trips; ++t) {
        if (at.major < segments) {                           // wave-uniform
            const uint32_t wx = at.minor * (uint32_t)kSsimStripWindows + lane;
            const uint32_t bx = min(wx, bw - 1u);
            const bool column = lane < (uint32_t)kSsimStripWindows && wx + 1u < bw;
            const uint32_t by0 = at.major * (uint32_t)kSsimSegmentRows;
            const uint32_t rows = min((uint32_t)kSsimSegmentRows + 1u, bh - by0);          // block rows: at least 2
            size_t aOff = (size_t)by0 * 4u * aPitch + (size_t)bx * 16u, bOff = (size_t)by0 * 4u * bPitch + (size_t)bx * 16u;
            uint32_t above[kSsimSums];
#pragma unroll
            for (int i = 0; i < kSsimSums; ++i) above[i] = 0u;
#pragma unroll 1
            for (uint32_t r = 0; r < rows; ++r) {
                uint32_t pair[kSsimSums];
                ssim_block<kWide>(a, aPitch, aOff, b, bPitch, bOff, pair);
                aOff += 4u * aPitch;
                bOff += 4u * bPitch;
#pragma unroll
                for (int i = 0; i < kSsimSums; ++i) pair[i] += (uint32_t)__shfl_down((int)pair[i], 1, 64);
                if (r > 0u) {                                // wave-uniform
                    int32_t m = 0x7fffffff;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int32_t q = ssim_q(above[3 * c] + pair[3 * c], above[3 * c + 1] + pair[3 * c + 1],
                                                 above[3 * c + 2] + pair[3 * c + 2], column);
                        if (column) sum[c] += (unsigned long long)(long long)q;
                        if ((channelMask >> c) & 1u) m = min(m, q);
                    }
                    const uint32_t wy = by0 + r - 1u;
                    const uint32_t bin = (uint32_t)max(m, 0) >> 18;
                    const unsigned long long key = ((unsigned long long)(uint32_t)(m + kSsimOne) << 32) | ((unsigned long long)wy << 16) | wx;
                    if (column) best = min(best, key);
                    identical += (uint32_t)__popcll(__ballot(column && bin == 64u));
                    if (column && bin != 64u) atomicAdd(&bins[bin], 1u);
                }
#pragma unroll
                for (int i = 0; i < kSsimSums; ++i) above[i] = pair[i];
            }
        }
        at.advance(stepSegment, stepStrip, strips);
    }

#pragma unroll
    for (int c = 0; c < 4; ++c) sum[c] = wave_sum_u64(sum[c]);
    best = wave_min_u64(best);
    if (lane == 0u) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[c][wave] = sum[c];
        part[4][wave] = best;
        if (identical != 0u) atomicAdd(&bins[64], identical);
    }
    __syncthreads();
    // the record: windows, sum[4], hist[65], worst
    if (tid < 4u) {
        record_add(stats + 1 + tid, group_sum_u64(part[tid]));
    } else if (tid == 4u) {
        const unsigned long long s = group_min_u64(part[4]);
        if (s != ~0ull) atomicMin(stats + 5 + kSsimBins, s);
    } else if (tid == 5u) {
        if (blockIdx.x == 0) atomicAdd(stats, windows);      // onto the cleared word, or onto the record's own count
    }
    if (tid >= 64u && tid < 64u + (uint32_t)kSsimBins) {
        record_add(stats + 5 + (tid - 64u), bins[tid - 64u]);
    }
}

}  // namespace

// The clear (zeros, then all ones into `worst`), then one launch of the fixed grid.
hipError_t launch_frame_ssim(hipStream_t s, const lfg_frame &a, const lfg_frame &b, uint32_t channelMask, bool accumulate,
                             int deviceCus, void *stats) {
    const uint32_t bw = a.width >> 2, bh = a.height >> 2;
    if (bw < 2u || bh < 2u) return hipErrorInvalidValue;
    const bool wide = multiples_of_16(a.data, b.data, a.pitch, b.pitch);
    const unsigned long long windows = (unsigned long long)(bw - 1u) * (bh - 1u);
    const uint32_t strips = (bw - 1u + kSsimStripWindows - 1u) / kSsimStripWindows;
    const uint32_t segments = (bh - 1u + kSsimSegmentRows - 1u) / kSsimSegmentRows;
    RecordGrid g;                                            // an item is at most 63 x 8 windows
    if (!record_fixed_grid<uint32_t>(strips, segments, kSsimWaves, 1, kSsimGroupsPerCu, deviceCus,
                                     kSsimGroupWindows / (kSsimStripWindows * kSsimSegmentRows), g))
        return hipErrorInvalidValue;
    const RecordDivisor d = record_divisor(strips);
    hipError_t e = record_clear(s, stats, offsetof(lfg_frame_ssim_stats, worst), accumulate);
    if (e == hipSuccess && !accumulate) e = hipMemsetAsync((uint8_t *)stats + offsetof(lfg_frame_ssim_stats, worst), 0xFF, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const auto kernel = wide ? frame_ssim_kernel<true> : frame_ssim_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(kSsimThreads), 0, s, (const uint8_t *)a.data, (size_t)a.pitch,
                       (const uint8_t *)b.data, (size_t)b.pitch, bw, bh, strips, segments, d.magic, d.shift,
                       (uint32_t)(g.stride / strips), (uint32_t)(g.stride % strips), g.trips, channelMask, windows,
                       (unsigned long long *)stats);
    return hipGetLastError();
}

}  // namespace lfg
