// Device side of the kernels that reduce a frame to a small record of 64-bit words (pair_stats.hip, frame_diff.hip,
// frame_ssim.hip, levels.hip; their launch plans are lfg_record_plan.hpp's): a lane keeps its sums in registers, a wave adds
// them up, lane 0 of each wave leaves them in LDS, and after one barrier one thread per sum adds the workgroup's share to
// the record with an atomic whose result is unused.  Histograms go through workgroup-private 32-bit LDS bins, merged the same
// way.  Everything is an integer: neither the walk nor the order of the atomics changes a result.  gfx950 only.
#pragma once

#include "lfg_device.hpp"

namespace lfg {

// The clear of the record in front of a launch, unless the call accumulates onto what the record holds.
inline hipError_t record_clear(hipStream_t s, void *stats, size_t bytes, bool accumulate) {
    return accumulate ? hipSuccess : hipMemsetAsync(stats, 0, bytes, s);
}

// The sum / the smallest of a wave's 64 values, in every lane.
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// The workgroup's value from what lane 0 of each wave left in LDS, behind the barrier.
template <int kWaves>
__device__ __forceinline__ unsigned long long group_sum_u64(const unsigned long long (&part)[kWaves]) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += part[w];
    return s;
}

template <int kWaves>
__device__ __forceinline__ unsigned long long group_min_u64(const unsigned long long (&part)[kWaves]) {
    unsigned long long s = ~0ull;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s = min(s, part[w]);
    return s;
}

// A workgroup's share of one word of the record.  An empty share adds nothing; result unused: global_atomic_add_x2.
__device__ __forceinline__ void record_add(unsigned long long *word, unsigned long long share) {
    if (share != 0ull) atomicAdd(word, share);
}

// The one hazard of an LDS histogram: all 64 lanes of a wave may hit one word -- flat content, a uniform offset, an alpha
// channel that is 255 everywhere -- and ds_add_u32 to one address serialises.  `all` is the ballot of the lanes that count
// something (`counts`; the caller skips the call where it is 0, so the whole wave must arrive here).  Where all of them
// share the bin of the first, one lane adds their number; only otherwise does every one of them add 1 to its own bin.
// `holds`: the lane's `bin` may be compared -- the lanes of `all`, or more of them where no other lane can hold the bin of
// one that counts.
__device__ __forceinline__ void bins_add(uint32_t *__restrict__ bins, uint32_t bin, bool holds, bool counts, unsigned long long all,
                                         uint32_t lane) {
    const int lead = __ffsll((long long)all) - 1;
    const uint32_t shared = (uint32_t)__builtin_amdgcn_readlane((int)bin, lead);
    if (__ballot(holds && bin == shared) == all) {           // wave-uniform
        if ((int)lane == lead) atomicAdd(&bins[shared], (uint32_t)__popcll(all));
    } else if (counts) {
        atomicAdd(&bins[bin], 1u);
    }
}

}  // namespace lfg
