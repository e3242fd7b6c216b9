// motion_subpel.hip -- quarter-pixel refinement of an integer vector field (lfg_motion_subpel, include/linuxfg_hip.h).
// No reference counterpart; opt-in, between the last integer stage and the sub-pixel compensated route
// (interpolate_subpel.hip).  tests/subpel_model.c restates the definition on the CPU.
//
// One launch of the window-cost family's shape and its masked cost (lfg_window_cost.hpp), on a sample that is this file's own.
// curr's (2R + 1)^2 window and the (2R + 3)^2 prev texels around q + v are read once, prev's split into its even and odd
// channels (16-bit halves of two registers per texel).  A candidate w = 4v + d, d in [-3, 3]^2, samples prev at
// r + v + (d >> 2) with the quarters (d & 3): per axis that is the three texels at -1, 0, +1 of the block with the weights
// (-d, 4 + d, 0) for d < 0 and (0, 4 - d, d) otherwise, so every candidate is one 3 x 3 weighted sum with STATIC register
// indices and the weights as data -- five of the nine weights are zero, which costs multiply-adds and saves the scratch
// that a data-dependent index into the block would mean.  Sums stay below 255 * 16 + 8 per half.
//
// Stage 1 takes the nine half-pixel candidates, stage 2 the nine around its winner (the winner itself again: 18
// evaluations for the 17 distinct candidates, one loop body for both stages).  The key (cost, |d|^2, dy, dx) is one uint64 whose
// minimum wins: the order is total.  Both loops run their constant nine trips, not unrolled, so the code stays one
// candidate long.  Every texel load comes unconditionally from a clamped position (lfg_device.hpp: texel_or_zero).  No
// atomics, no scratch, no data-dependent loop bounds.
#include "lfg_window_cost.hpp"

namespace lfg {
namespace {

// The three weights of one axis for the offset d in [-3, 3], on the texels at -1, 0, +1.
__device__ __forceinline__ void axis_weights(int d, uint32_t (&w)[3]) {
    w[0] = d < 0 ? (uint32_t)(-d) : 0u;
    w[1] = d < 0 ? (uint32_t)(4 + d) : (uint32_t)(4 - d);
    w[2] = d < 0 ? 0u : (uint32_t)d;
}

template <int R>
struct SubpelWindow {
    static constexpr int D = 2 * R + 1, E = D + 2;
    uint32_t cw[D * D];          // curr's window
    uint32_t pe[E * E], po[E * E];   // prev's block: channels 0 and 2 / 1 and 3 in 16-bit halves
    uint32_t inWin;              // bit j * D + i: window texel (i, j) lies inside the image

    // cost(4v + (dx, dy)) as the key (cost, |d|^2, dy, dx); all ones where the candidate leaves [-508, 508]
    __device__ __forceinline__ uint64_t key(Mv v4, int dx, int dy) const {
        uint32_t wx[3], wy[3], w9[9];
        axis_weights(dx, wx);
        axis_weights(dy, wy);
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int a = 0; a < 3; ++a) w9[b * 3 + a] = wx[a] * wy[b];
        uint32_t cost = 0u;
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int i = 0; i < D; ++i) {
                uint32_t even = 0x00080008u, odd = 0x00080008u;
#pragma unroll
                for (int b = 0; b < 3; ++b)
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        even += pe[(j + b) * E + i + a] * w9[b * 3 + a];
                        odd += po[(j + b) * E + i + a] * w9[b * 3 + a];
                    }
                cost = window_add(cw, inWin, j * D + i, ((even >> 4) & 0x00FF00FFu) | (((odd >> 4) & 0x00FF00FFu) << 8), cost);
            }
        const int wqx = v4.x + dx, wqy = v4.y + dy;
        const bool inRange = wqx >= -kMvqLimit && wqx <= kMvqLimit && wqy >= -kMvqLimit && wqy <= kMvqLimit;
        return inRange ? ((uint64_t)cost << 32) | mvq_delta_key(dx, dy) : ~0ull;
    }
};

template <int R>
__global__ __launch_bounds__(kWinBlockX * kWinBlockY) void motion_subpel_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mvIn, size_t mvInPitch, uint8_t *__restrict__ mvqOut, size_t mvqOutPitch, int W, int H) {
    constexpr int D = 2 * R + 1, E = D + 2;
    const int x = (int)blockIdx.x * kWinBlockX + (int)threadIdx.x, y = (int)blockIdx.y * kWinBlockY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    Mv v = mv_unpack(*reinterpret_cast<const uint16_t *>(mvIn + (size_t)y * mvInPitch + (size_t)x * 2u));
    v.x = max(v.x, -127); v.y = max(v.y, -127);              // a byte of -128 is read as -127

    SubpelWindow<R> win;
    win.inWin = 0u;
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int rx = x + i - R, ry = y + j - R;
            win.inWin |= (rx >= 0 && rx < W && ry >= 0 && ry < H ? 1u : 0u) << (j * D + i);
            win.cw[j * D + i] = texel_or_zero(curr, currPitch, rx, ry, W, H);
        }
    // block texel (i, j) = prev at window texel (i - 1, j - 1) + v: a tap at -1, 0, +1 of window texel (i, j) is block index + 0, 1, 2
#pragma unroll
    for (int j = 0; j < E; ++j)
#pragma unroll
        for (int i = 0; i < E; ++i) {
            const uint32_t p = texel_or_zero(prev, prevPitch, x + i - R - 1 + v.x, y + j - R - 1 + v.y, W, H);
            win.pe[j * E + i] = p & 0x00FF00FFu;
            win.po[j * E + i] = (p >> 8) & 0x00FF00FFu;
        }

    const Mv v4{4 * v.x, 4 * v.y};
    uint64_t best = ~0ull;                                   // stage 1: 4v + (2a, 2b); (0, 0) is always in range
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
        const uint64_t key = win.key(v4, 2 * (k % 3 - 1), 2 * (k / 3 - 1));
        best = key < best ? key : best;
    }
    const Mv h = mvq_delta_decode((uint32_t)best);
    best = ~0ull;                                            // stage 2: h + (a, b), h among them
#pragma unroll 1
    for (int k = 0; k < 9; ++k) {
        const uint64_t key = win.key(v4, h.x + k % 3 - 1, h.y + k / 3 - 1);
        best = key < best ? key : best;
    }
    const Mv d = mvq_delta_decode((uint32_t)best);
    *reinterpret_cast<uint32_t *>(mvqOut + (size_t)y * mvqOutPitch + (size_t)x * 4u) = mvq_word(v4.x + d.x, v4.y + d.y);
}

}  // namespace

hipError_t launch_motion_subpel(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvIn,
                                const lfg_frame &mvqOut, int radius) {
    return window_cost_launch(motion_subpel_kernel<0>, motion_subpel_kernel<1>, motion_subpel_kernel<2>, radius, s, prev, curr, mvIn, mvqOut);
}

}  // namespace lfg
