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
//   * Items go to waves in a grid-stride walk of a FIXED grid (kSsimGroupsPerCu workgroups of kSsimWaves waves per CU); every
//     wave runs the host's `trips`, and whether an item exists, how many block rows it has and which lanes hold a window follow
//     from the sizes alone.  The one data-dependent branch is wave-uniform: where N = D in every window of the wave (identical
//     content: Q = 2^24) the 25 steps of the restoring division are skipped for that channel.
//   * D < 2^58 and |N| <= D, so the division shifts a remainder below D left by one bit 24 times inside 64 bits.
//   * The histogram: bin 64 (identical windows) is counted by ballot and population count into a wave-uniform scalar, as
//     frame_diff.hip counts its zeros; the other bins go to a workgroup-private LDS histogram of 32-bit bins.  One merge per
//     workgroup: 64-bit atomic adds of the sums and the non-empty bins, one 64-bit atomic minimum of the key.
// No float anywhere.  All 71 results are integers: neither the walk nor the order of the atomics changes them.
#include <algorithm>

#include "lfg_internal.hpp"
#include "lfg_device.hpp"

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

    // this wave's first item as (segment, strip): first / strips through the host's multiplier (launch_frame_ssim: exact for
    // first < 2^31), then the step between its items, gridDim.x * kSsimWaves of them, as segments and a rest
    const uint32_t first = blockIdx.x * (uint32_t)kSsimWaves + wave;
    uint32_t segment = (uint32_t)(((unsigned long long)first * divMagic) >> divShift);
    uint32_t strip = first - segment * strips;

    unsigned long long sum[4] = {0ull, 0ull, 0ull, 0ull};    // this lane's windows, two's complement
    unsigned long long best = ~0ull;                         // this lane's smallest key
    uint32_t identical = 0u;                                 // this wave's windows in bin 64 (wave-uniform)
    for (uint32_t t = 0; t < trips; ++t) {
        if (segment < segments) {                            // wave-uniform
            const uint32_t wx = strip * (uint32_t)kSsimStripWindows + lane;
            const uint32_t bx = min(wx, bw - 1u);
            const bool column = lane < (uint32_t)kSsimStripWindows && wx + 1u < bw;
            const uint32_t by0 = segment * (uint32_t)kSsimSegmentRows;
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
        strip += stepStrip;
        segment += stepSegment;
        if (strip >= strips) { strip -= strips; ++segment; }
    }

#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum[c] += __shfl_xor(sum[c], o, 64);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    if (lane == 0u) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[c][wave] = sum[c];
        part[4][wave] = best;
        if (identical != 0u) atomicAdd(&bins[64], identical);
    }
    __syncthreads();
    // the record: windows, sum[4], hist[65], worst.  Empty sums and bins add nothing; results unused
    if (tid < 4u) {
        unsigned long long s = 0ull;
#pragma unroll
        for (int w = 0; w < kSsimWaves; ++w) s += part[tid][w];
        if (s != 0ull) atomicAdd(stats + 1 + tid, s);
    } else if (tid == 4u) {
        unsigned long long s = ~0ull;
#pragma unroll
        for (int w = 0; w < kSsimWaves; ++w) s = min(s, part[4][w]);
        if (s != ~0ull) atomicMin(stats + 5 + kSsimBins, s);
    } else if (tid == 5u) {
        if (blockIdx.x == 0) atomicAdd(stats, windows);      // onto the cleared word, or onto the record's own count
    }
    if (tid >= 64u && tid < 64u + (uint32_t)kSsimBins) {
        const uint32_t n = bins[tid - 64u];
        if (n != 0u) atomicAdd(stats + 5 + (tid - 64u), (unsigned long long)n);
    }
}

}  // namespace

// The clear unless the call accumulates (zeros, then all ones into `worst`), then one launch.  Workgroups: kSsimGroupsPerCu per
// CU, never more than there are items -- and never so few that one of them would see more than kSsimGroupWindows windows.
hipError_t launch_frame_ssim(hipStream_t s, const lfg_frame &a, const lfg_frame &b, uint32_t channelMask, bool accumulate,
                             int deviceCus, void *stats) {
    const uint32_t bw = a.width >> 2, bh = a.height >> 2;
    if (bw < 2u || bh < 2u) return hipErrorInvalidValue;
    const bool wide = (((uintptr_t)a.data | (uintptr_t)b.data | (uintptr_t)a.pitch | (uintptr_t)b.pitch) % 16u) == 0;
    const unsigned long long windows = (unsigned long long)(bw - 1u) * (bh - 1u);
    const uint32_t strips = (bw - 1u + kSsimStripWindows - 1u) / kSsimStripWindows;
    const uint32_t segments = (bh - 1u + kSsimSegmentRows - 1u) / kSsimSegmentRows;
    const unsigned long long items = (unsigned long long)strips * segments;
    // a workgroup takes at most items / (grid * kSsimWaves) + 1 trips of kSsimWaves items of 63 x 8 windows each
    const unsigned long long perTrip = (unsigned long long)kSsimWaves * kSsimStripWindows * kSsimSegmentRows;
    const unsigned long long atLeast = items / (kSsimWaves * (kSsimGroupWindows / perTrip - 1ull)) + 1ull;
    const unsigned long long fixed = (unsigned long long)std::max(deviceCus, 1) * kSsimGroupsPerCu;
    const unsigned long long grid = std::max(std::min((items + kSsimWaves - 1) / kSsimWaves, fixed), atLeast);
    const unsigned long long stride = grid * kSsimWaves;
    const unsigned long long trips = (items + stride - 1) / stride;
    if (stride + items > 0x80000000ull || trips > 0xffffffffull) return hipErrorInvalidValue;      // (no frame a device holds comes near)
    // n / strips for every n < 2^31 as (n * magic) >> shift: with 2^(l-1) < strips <= 2^l, magic = ceil(2^(31+l) / strips)
    // <= 2^32 and shift = 31 + l <= 63 (Granlund and Montgomery 1994, theorem 4.2); n * magic < 2^63
    uint32_t l = 0;
    while ((1ull << l) < (unsigned long long)strips) ++l;
    const uint32_t divShift = 31u + l;
    const unsigned long long divMagic = ((1ull << divShift) + strips - 1ull) / strips;
    if (!accumulate) {
        hipError_t e = hipMemsetAsync(stats, 0, offsetof(lfg_frame_ssim_stats, worst), s);
        if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)stats + offsetof(lfg_frame_ssim_stats, worst), 0xFF, sizeof(uint64_t), s);
        if (e != hipSuccess) return e;
    }
    const auto kernel = wide ? frame_ssim_kernel<true> : frame_ssim_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(kSsimThreads), 0, s, (const uint8_t *)a.data, (size_t)a.pitch,
                       (const uint8_t *)b.data, (size_t)b.pitch, bw, bh, strips, segments, divMagic, divShift,
                       (uint32_t)(stride / strips), (uint32_t)(stride % strips), (uint32_t)trips, channelMask, windows,
                       (unsigned long long *)stats);
    return hipGetLastError();
}

}  // namespace lfg
