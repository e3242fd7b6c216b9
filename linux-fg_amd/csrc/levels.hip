// levels.hip -- level matching: what lets the stages keep their vectors through a fade, a flash or an exposure change
// (lfg_frame_histogram, lfg_levels_match, lfg_levels_apply, include/linuxfg_hip.h).  No reference
// counterpart; opt-in.  tests/levels_model.py restates the definitions on the CPU, lfg_levels.hpp holds the rule both sides run.
//
// frame_histogram_kernel  per channel the number of pixels at each of the 256 levels.  4 bytes read per pixel, nothing
//                         written but the record.
// levels_match_kernel     one workgroup: both records' running sums, both maps by bisection, the gate.
// levels_apply_kernel     a map through every pixel of a frame, its 768 bytes staged (and for LFG_LEVELS_AT combined) in LDS.
//
// The histogram is a record kernel: its row layout, its rectangle and its refusal are lfg_record_plan.hpp's (hist_row,
// hist_grid), the LDS bins' one-lane add and the merge lfg_record.hpp's.  What is this file's:
//   * The workgroup is a rectangle of lanes, bx wide and 1024 / bx high, so a wave lies in ONE row, neither the walk nor a
//     lane's address takes a division, and every lane of a wave runs the same trips: the ballots see the whole wave.
//   * An item is four pixels of one row through one 16-byte load where the row's base allows it, one pixel through a dword
//     load otherwise.  With a pitch that is a multiple of 16 every row has the same 0 .. 3 pixels in front of its first
//     16-byte boundary and the same 0 .. 3 behind its last: those are items of one pixel at the end of the row's items, in
//     the same launch.  With any other pitch every item is one pixel.
//   * The one-lane add is asked per pixel AND channel, because alpha is uniform in nearly every frame while colour is not.
// No float anywhere but the one conversion of LFG_LEVELS_AT's factor on the host.  All results are integers: neither the walk
// nor the order of the atomics changes them.
#include <algorithm>

#include "lfg_internal.hpp"
#include "lfg_record.hpp"
#include "lfg_record_plan.hpp"
#include "lfg_levels.hpp"

namespace lfg {
namespace {

constexpr int kHistThreads = 1024;                          // 16 waves: one LDS histogram and one merge for all of them
constexpr int kHistGroupsPerCu = 1;                         // workgroups per CU of the fixed grid: every one merges 1,024 bins
constexpr int kHistUnroll = 2;                              // rows of a lane per trip of the walk
constexpr int kHistBins = 4 * kLevels;
// The most pixels one workgroup may see in a launch (launch_frame_histogram sizes the grid by it): what keeps a 32-bit bin exact.
constexpr unsigned long long kHistGroupPixels = 1ull << 31;

// One pixel word of every lane of the wave that has one (`valid`) into the workgroup's bins.
__device__ __forceinline__ void count_word(uint32_t *__restrict__ bins, uint32_t p, bool valid, uint32_t lane) {
    const unsigned long long all = __ballot(valid);
    if (all == 0ull) return;                                 // wave-uniform
#pragma unroll
    for (int c = 0; c < 4; ++c) bins_add(bins + c * kLevels, (p >> (8 * c)) & 0xffu, valid, valid, all, lane);
}

__global__ __launch_bounds__(kHistThreads) void frame_histogram_kernel(
        const uint8_t *__restrict__ frame, size_t pitch, uint32_t H, HistRow r, uint32_t lgBx, unsigned long long pixels,
        unsigned long long *__restrict__ stats) {
    __shared__ uint32_t bins[kHistBins];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t i = tid; i < (uint32_t)kHistBins; i += kHistThreads) bins[i] = 0u;
    __syncthreads();

    const uint32_t bx = 1u << lgBx, by = (uint32_t)kHistThreads >> lgBx;
    const uint32_t tx = tid & (bx - 1u), ty = tid >> lgBx;                      // ty is the same for a wave's lanes: bx >= 64
    const unsigned long long rowStep = (unsigned long long)gridDim.y * by * kHistUnroll;
    const unsigned long long gStep = (unsigned long long)gridDim.x * bx;
    for (unsigned long long g0 = (unsigned long long)blockIdx.x * bx; g0 < r.itemsX; g0 += gStep) {
        const unsigned long long g = g0 + tx;
        const bool inRow = g < r.itemsX, wide = g < r.wideItems;
        const uint32_t x = hist_item_x(r, (uint32_t)g, wide);                   // the item's first pixel
        for (unsigned long long y0 = (unsigned long long)blockIdx.y * by * kHistUnroll; y0 < H; y0 += rowStep) {
            uint32_t p[kHistUnroll][4];
            bool item[kHistUnroll];
#pragma unroll
            for (int k = 0; k < kHistUnroll; ++k) {
                const unsigned long long y = y0 + (unsigned long long)k * by + ty;
                item[k] = inRow && y < H;
                p[k][0] = p[k][1] = p[k][2] = p[k][3] = 0u;
                if (item[k]) {
                    const uint8_t *__restrict__ t = frame + (size_t)y * pitch + (size_t)x * 4u;
                    if (wide) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(t);
                        p[k][0] = v.x; p[k][1] = v.y; p[k][2] = v.z; p[k][3] = v.w;
                    } else {
                        p[k][0] = *reinterpret_cast<const uint32_t *>(t);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kHistUnroll; ++k) {
                count_word(bins, p[k][0], item[k], lane);
#pragma unroll
                for (int i = 1; i < 4; ++i) count_word(bins, p[k][i], item[k] && wide, lane);
            }
        }
    }

    __syncthreads();
    // the record: pixels, hist[4][256]
    for (uint32_t i = tid; i < (uint32_t)kHistBins; i += kHistThreads) record_add(stats + 1 + i, bins[i]);
    if (tid == 0u && blockIdx.x == 0 && blockIdx.y == 0) atomicAdd(stats, pixels);   // onto the cleared word, or the record's own count
}

// ---- the maps

constexpr int kMatchThreads = kLevels;

__global__ __launch_bounds__(kMatchThreads) void levels_match_kernel(const unsigned long long *__restrict__ from,
                                                                     const unsigned long long *__restrict__ to, int minShift16,
                                                                     uint8_t *__restrict__ map) {
    __shared__ uint64_t cdf[2][kLevelChannels][kLevels];     // [0]: from, [1]: to; the histograms, then their running sums
    __shared__ unsigned long long part[kMatchThreads / 64];
    const uint32_t v = threadIdx.x;
    uint64_t own[kLevelChannels];                            // from's histogram at this thread's level
#pragma unroll
    for (int c = 0; c < kLevelChannels; ++c) {
        own[c] = from[1 + c * kLevels + v];
        cdf[0][c][v] = own[c];
        cdf[1][c][v] = to[1 + c * kLevels + v];
    }
    __syncthreads();
    if (v < 2u * kLevelChannels) {                           // six short serial sums: 256 adds each
        uint64_t *h = cdf[v / kLevelChannels][v % kLevelChannels];
        levels_cdf(h, h);
    }
    __syncthreads();
    uint32_t fwd[kLevelChannels], inv[kLevelChannels];
    uint64_t shift = 0;
#pragma unroll
    for (int c = 0; c < kLevelChannels; ++c) {
        fwd[c] = levels_rank(cdf[1][c], cdf[0][c][v]);
        inv[c] = levels_rank(cdf[0][c], cdf[1][c][v]);
        shift += levels_shift(own[c], fwd[c], v);
    }
    shift = wave_sum_u64(shift);
    if ((v & 63u) == 0u) part[v >> 6] = shift;
    __syncthreads();
    const uint64_t shiftSum = group_sum_u64(part);
    const uint64_t pixels = from[0];
    const bool active = levels_active(pixels, to[0], shiftSum, minShift16);
    uint8_t *forward = map + kMapHeadBytes, *inverse = forward + kLevelChannels * kLevels;
#pragma unroll
    for (int c = 0; c < kLevelChannels; ++c) {
        forward[c * kLevels + v] = (uint8_t)(active ? fwd[c] : v);
        inverse[c * kLevels + v] = (uint8_t)(active ? inv[c] : v);
    }
    if (v == 0u) {
        unsigned long long *head = reinterpret_cast<unsigned long long *>(map);
        head[0] = pixels;
        head[1] = shiftSum;
        head[2] = active ? 1ull : 0ull;                      // active, then reserved = 0
    }
}

// ---- a map through a frame

constexpr int kApplyThreads = 256;
constexpr int kApplyGroups = 2048;                          // workgroups of the grid at most: each stages the table once

// `in` and `out` may be the same frame: every pixel is read before it is written, by the lane that writes it.
// wideItems: the 16-byte items of a row (the host passes 0 unless base and pitch of both frames are multiples of 16); the
// W - 4 * wideItems pixels behind them are items of one pixel.
__global__ __launch_bounds__(kApplyThreads) void levels_apply_kernel(const uint8_t *in, size_t inPitch, uint8_t *out, size_t outPitch,
                                                                     uint32_t W, uint32_t H, uint32_t wideItems,
                                                                     const uint8_t *__restrict__ map, int mode, int tq) {
    __shared__ uint8_t table[kLevelChannels * kLevels];
    const uint8_t *__restrict__ forward = map + kMapHeadBytes, *__restrict__ inverse = forward + kLevelChannels * kLevels;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kLevelChannels * kLevels); i += kApplyThreads)
        table[i] = mode == LFG_LEVELS_FORWARD ? forward[i] : (uint8_t)levels_at(inverse[i], i & 255u, tq);
    __syncthreads();
    const uint32_t itemsX = wideItems + (W - 4u * wideItems);
    for (unsigned long long g = (unsigned long long)blockIdx.x * kApplyThreads + threadIdx.x; g < itemsX;
         g += (unsigned long long)gridDim.x * kApplyThreads) {
        const bool wide = g < wideItems;
        const size_t xBytes = wide ? (size_t)g * 16u : ((size_t)wideItems * 4u + ((size_t)g - wideItems)) * 4u;
        for (unsigned long long y = blockIdx.y; y < H; y += gridDim.y) {
            const uint8_t *src = in + (size_t)y * inPitch + xBytes;
            uint8_t *dst = out + (size_t)y * outPitch + xBytes;
            if (wide) {
                uint4 q = *reinterpret_cast<const uint4 *>(src);
                q.x = levels_texel(table, q.x); q.y = levels_texel(table, q.y);
                q.z = levels_texel(table, q.z); q.w = levels_texel(table, q.w);
                store_16_guarded(dst, q);
            } else {
                *reinterpret_cast<uint32_t *>(dst) = levels_texel(table, *reinterpret_cast<const uint32_t *>(src));
            }
        }
    }
}

}  // namespace

// The clear, then one launch of the fixed grid.
hipError_t launch_frame_histogram(hipStream_t s, const lfg_frame &frame, bool accumulate, int deviceCus, void *stats) {
    const uint32_t W = frame.width, H = frame.height;
    const HistRow r = hist_row(frame.data, frame.pitch, W);
    HistGrid g;
    if (!hist_grid(r.itemsX, H, kHistThreads, kHistUnroll, kHistGroupsPerCu, deviceCus, kHistGroupPixels, g)) return hipErrorInvalidValue;
    const hipError_t e = record_clear(s, stats, sizeof(lfg_frame_histogram_stats), accumulate);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(frame_histogram_kernel, dim3(g.groupsX, g.groupsY), dim3(kHistThreads), 0, s, (const uint8_t *)frame.data,
                       (size_t)frame.pitch, H, r, g.lgBx, (unsigned long long)W * H, (unsigned long long *)stats);
    return hipGetLastError();
}

hipError_t launch_levels_match(hipStream_t s, const void *from, const void *to, int minShift16, void *map) {
    hipLaunchKernelGGL(levels_match_kernel, dim3(1), dim3(kMatchThreads), 0, s, (const unsigned long long *)from,
                       (const unsigned long long *)to, minShift16, (uint8_t *)map);
    return hipGetLastError();
}

hipError_t launch_levels_apply(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const void *map, int mode, int tq) {
    const uint32_t W = in.width, H = in.height;
    const uint32_t wideItems = wide_columns(multiples_of_16(in.data, out.data, in.pitch, out.pitch), W) / 4u;
    const unsigned long long itemsX = (unsigned long long)wideItems + (W - 4u * wideItems);
    const unsigned long long groupsX = std::min((itemsX + kApplyThreads - 1) / kApplyThreads, (unsigned long long)kApplyGroups);
    const unsigned long long groupsY = std::min<unsigned long long>(H, std::max((unsigned long long)kApplyGroups / groupsX, 1ull));
    hipLaunchKernelGGL(levels_apply_kernel, dim3((uint32_t)groupsX, (uint32_t)groupsY), dim3(kApplyThreads), 0, s,
                       (const uint8_t *)in.data, (size_t)in.pitch, (uint8_t *)out.data, (size_t)out.pitch, W, H, wideItems,
                       (const uint8_t *)map, mode, tq);
    return hipGetLastError();
}

}  // namespace lfg
