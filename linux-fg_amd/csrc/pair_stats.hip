// pair_stats.hip -- scene-cut detection (lfg_pair_match, lfg_cut_fallback, include/linuxfg_hip.h).  No reference counterpart;
// opt-in, around either interpolator.  tests/pair_model.py restates both definitions on the CPU.
//
// pair_match_kernel   how well the vectors explain the pair: the compensated interpolator's match gate (lfg_mc.hpp:
//                     matched) evaluated at every pixel, counted, and the SADs summed.  One launch behind a clear of the record.
// cut_fallback_kernel reads that record on the device; a pair that is no cut costs the launch and one load per wave, a cut
//                     copies prev or curr over every output.  The host never learns the verdict here.
//
// pair_match_kernel is a record kernel with a FIXED grid (lfg_record_plan.hpp: pair_grid), not one workgroup per tile: a
// workgroup's cost at the end is two 64-bit atomics into the same two words, and at 4K a grid of tiles would be 32,400 of
// them.  Each workgroup walks the 64 x 4 tiles blockIdx.x, blockIdx.x + gridDim.x, ...; a wave is 64 pixels of one row.  Per
// tile every lane loads its vector, then curr and the gathered prev texel -- unconditionally, from clamped positions, the
// outside value selected afterwards (lfg_device.hpp: texel_or_zero), two tiles per trip so that four waves keep sixteen loads
// in flight.  Partial sums stay in registers: the SAD per lane, the matched count per wave (ballot + population count, a
// scalar).  Both are 64-bit, so no frame size can wrap them.  The wave sum and the merge are lfg_record.hpp's.
// All three results are integers: neither the walk nor the order of the atomics changes them.
//
// Traffic per pixel: 2 (mv) + 4 (curr) + 4 (gathered prev) = 10 bytes, 83 MB at 4K.
#include <algorithm>

#include "lfg_internal.hpp"
#include "lfg_record.hpp"
#include "lfg_record_plan.hpp"
#include "lfg_vector_word.hpp"

namespace lfg {
namespace {

constexpr int kPairBlockX = 64, kPairBlockY = 4;             // a wave is 64 pixels of one row
constexpr int kPairGroupsPerCu = 8;                         // workgroups per CU of the fixed grid
constexpr int kPairUnroll = 2;                               // tiles per trip of the walk

// The vector and curr's texel of pixel (x, y) of the tile walk; (x, y) may lie outside the image (a partial tile, or no tile
// at all): the loads then come from the clamped position, and the caller leaves the pixel out.
__device__ __forceinline__ void pair_loads(const uint8_t *__restrict__ curr, size_t currPitch, const uint8_t *__restrict__ mv,
                                           size_t mvPitch, int W, int H, int x, int y, uint32_t &vec, uint32_t &c) {
    const int cx = min(x, W - 1), cy = min(y, H - 1);
    vec = *reinterpret_cast<const uint16_t *>(mv + (size_t)cy * mvPitch + (size_t)cx * 2u);
    c = *reinterpret_cast<const uint32_t *>(curr + (size_t)cy * currPitch + (size_t)cx * 4u);
}

__global__ __launch_bounds__(kPairBlockX * kPairBlockY) void pair_match_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, int W, int H, uint32_t tilesX, uint32_t tiles, uint32_t matchSad,
        unsigned long long *__restrict__ stats) {
    __shared__ unsigned long long part[2][kPairBlockY];
    unsigned long long sad = 0ull;                           // this lane's pixels
    unsigned long long hits = 0ull;                          // this wave's pixels (wave-uniform)
    for (uint32_t t0 = blockIdx.x; t0 < tiles; t0 += gridDim.x * kPairUnroll) {
        int x[kPairUnroll], y[kPairUnroll];
        uint32_t vec[kPairUnroll], c[kPairUnroll], p[kPairUnroll];
        bool inTile[kPairUnroll];
#pragma unroll
        for (int k = 0; k < kPairUnroll; ++k) {
            const uint32_t t = t0 + (uint32_t)k * gridDim.x;
            // (a tile past the last one: every lane outside the image, loads from the clamped corner)
            x[k] = t < tiles ? (int)(t % tilesX) * kPairBlockX + (int)threadIdx.x : W;
            y[k] = t < tiles ? (int)(t / tilesX) * kPairBlockY + (int)threadIdx.y : H;
            inTile[k] = x[k] < W && y[k] < H;
            pair_loads(curr, currPitch, mv, mvPitch, W, H, x[k], y[k], vec[k], c[k]);
        }
#pragma unroll
        for (int k = 0; k < kPairUnroll; ++k) {
            const Mv v = mv_unpack((uint16_t)vec[k]);
            p[k] = texel_or_zero(prev, prevPitch, min(x[k], W - 1) + v.x, min(y[k], H - 1) + v.y, W, H);
        }
#pragma unroll
        for (int k = 0; k < kPairUnroll; ++k) {
            // the match gate (lfg_mc.hpp: matched), inline: its texels were loaded a loop ahead, and the SAD itself is summed
            const uint32_t s = __builtin_amdgcn_sad_u8(c[k], p[k], 0u);
            sad += inTile[k] ? s : 0u;
            hits += (unsigned long long)__popcll(__ballot(inTile[k] && s <= matchSad));
        }
    }
    sad = wave_sum_u64(sad);
    if (threadIdx.x == 0) { part[0][threadIdx.y] = hits; part[1][threadIdx.y] = sad; }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        if (blockIdx.x == 0) stats[0] = (unsigned long long)W * (unsigned long long)H;
        atomicAdd(stats + 1, group_sum_u64(part[0]));        // results unused: two global_atomic_add_x2
        atomicAdd(stats + 2, group_sum_u64(part[1]));
    }
}

constexpr int kCutThreads = 256;
constexpr int kCutUnroll = 4;                                // dwords in flight per lane

// Where each output comes from, by value: one launch for every output of a call.
struct CutOutputs {
    uint8_t *data[LFG_MAX_FACTORS];
    uint32_t pitch[LFG_MAX_FACTORS];
    uint32_t fromCurr;                                       // bit i: outs[i] takes curr (factors[i] >= 0.5f), else prev
    uint32_t count;
};

__global__ __launch_bounds__(kCutThreads) void cut_fallback_kernel(
        const unsigned long long *__restrict__ stats, unsigned long long permille, const uint8_t *__restrict__ prev,
        size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch, int W, int H, CutOutputs outs) {
    // the record through a wave-uniform load: every wave decides for itself, no barrier, no LDS
    const unsigned long long pixels = stats[0], matched = stats[1];
    if (!(matched * 1000ull < permille * pixels)) return;
    // a cut: rows of all outputs, strided over the workgroups; a row in dwords, strided over the lanes
    const uint32_t rows = (uint32_t)H * outs.count;
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t i = r / (uint32_t)H, y = r % (uint32_t)H;
        const bool fromCurr = (outs.fromCurr >> i) & 1u;
        const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(fromCurr ? curr + (size_t)y * currPitch : prev + (size_t)y * prevPitch);
        uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(outs.data[i] + (size_t)y * outs.pitch[i]);
        for (int x0 = (int)threadIdx.x; x0 < W; x0 += kCutThreads * kCutUnroll) {
            uint32_t v[kCutUnroll];
#pragma unroll
            for (int k = 0; k < kCutUnroll; ++k) v[k] = src[min(x0 + k * kCutThreads, W - 1)];
#pragma unroll
            for (int k = 0; k < kCutUnroll; ++k)
                if (x0 + k * kCutThreads < W) dst[x0 + k * kCutThreads] = v[k];
        }
    }
}

}  // namespace

// The clear, then one launch of the fixed grid.
hipError_t launch_pair_match(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, int matchSad,
                             int deviceCus, void *stats) {
    const int W = (int)curr.width, H = (int)curr.height;
    const PairGrid g = pair_grid(curr.width, curr.height, kPairBlockX, kPairBlockY, kPairUnroll, kPairGroupsPerCu, deviceCus);
    const hipError_t e = record_clear(s, stats, sizeof(lfg_pair_stats), false);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pair_match_kernel, dim3(g.grid), dim3(kPairBlockX, kPairBlockY), 0, s, (const uint8_t *)prev.data,
                       (size_t)prev.pitch, (const uint8_t *)curr.data, (size_t)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch,
                       W, H, g.tilesX, g.tiles, (uint32_t)matchSad, (unsigned long long *)stats);
    return hipGetLastError();
}

hipError_t launch_cut_fallback(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const void *stats, int minMatchedPermille,
                               const lfg_frame *const *outs, const float *factors, int count, int deviceCus) {
    CutOutputs o{};
    o.count = (uint32_t)count;
    for (int i = 0; i < count; ++i) {
        o.data[i] = (uint8_t *)outs[i]->data;
        o.pitch[i] = outs[i]->pitch;
        if (!(factors[i] < 0.5f)) o.fromCurr |= 1u << i;
    }
    const uint32_t rows = curr.height * (uint32_t)count;
    const uint32_t grid = std::min<uint32_t>(rows, (uint32_t)std::max(deviceCus, 1) * 4u);
    hipLaunchKernelGGL(cut_fallback_kernel, dim3(grid), dim3(kCutThreads), 0, s, (const unsigned long long *)stats,
                       (unsigned long long)minMatchedPermille, (const uint8_t *)prev.data, (size_t)prev.pitch,
                       (const uint8_t *)curr.data, (size_t)curr.pitch, (int)curr.width, (int)curr.height, o);
    return hipGetLastError();
}

}  // namespace lfg
