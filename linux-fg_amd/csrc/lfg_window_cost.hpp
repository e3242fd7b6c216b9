// What the window-cost family shares (motion_refine.hip, motion_expand.hip, motion_subpel.hip).  Each chooses a vector per
// pixel q by the sum of v_sad_u8 over the (2R + 1)^2 window of curr around q against prev displaced by a candidate; window
// texels outside the image are skipped (bit clear in the kernel's `inWin`), prev outside the image reads as 0
// (lfg_device.hpp: texel_or_zero), and the smallest key (cost, |v|^2, vy, vx), one uint64, wins.  The order is total, so
// neither the order of evaluation nor the tiling changes a result.  tests/window_model.h restates the cost and the key.
// Only what has no loop lives here.  The window load, the gathered cost, the minimum over distinct candidates and prev's
// block were tried as functions of this header too: each changes the kernels' machine code, and motion_refine_kernel and
// motion_expand_kernel came out slower (profiles/window_fold_ab.txt), so those loops stay in the kernels.
#pragma once

#include "lfg_device.hpp"
#include "lfg_internal.hpp"
#include "lfg_vector_word.hpp"

namespace lfg {

constexpr int kWinBlockX = 64, kWinBlockY = 4;               // one thread per pixel; a wave is 64 pixels of one row

// cost plus the SAD of window texel k (cw[k]) against the packed texel p; cost as it is where texel k is outside the image
template <int N>
__device__ __forceinline__ uint32_t window_add(const uint32_t (&cw)[N], uint32_t inWin, int k, uint32_t p, uint32_t cost) {
    const uint32_t sum = __builtin_amdgcn_sad_u8(cw[k], p, cost);
    return (inWin >> k) & 1u ? sum : cost;
}

// One launch of a window-cost kernel on curr's pixels, the instantiation for the radius (0, 1, else 2), and its error.
using WindowCostKernel = void (*)(const uint8_t *, size_t, const uint8_t *, size_t, const uint8_t *, size_t, uint8_t *, size_t, int, int);
inline hipError_t window_cost_launch(WindowCostKernel r0, WindowCostKernel r1, WindowCostKernel r2, int radius, hipStream_t s,
                                     const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, const lfg_frame &out) {
    const int W = (int)curr.width, H = (int)curr.height;
    const dim3 block(kWinBlockX, kWinBlockY), grid((unsigned)((W + kWinBlockX - 1) / kWinBlockX), (unsigned)((H + kWinBlockY - 1) / kWinBlockY));
    hipLaunchKernelGGL(radius == 0 ? r0 : radius == 1 ? r1 : r2, grid, block, 0, s, (const uint8_t *)prev.data, (size_t)prev.pitch,
                       (const uint8_t *)curr.data, (size_t)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (uint8_t *)out.data,
                       (size_t)out.pitch, W, H);
    return hipGetLastError();
}

}  // namespace lfg
