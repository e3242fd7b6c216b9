// motion_expand.hip -- half-resolution motion carried to full size (lfg_frame_halve, lfg_motion_expand, include/linuxfg_hip.h).
// No reference counterpart; opt-in, between either estimator run on halved frames and everything that takes a vector field.
// tests/expand_model.c restates both definitions on the CPU.
//
// frame_halve_kernel: the pyramid's level rule (motion_pyramid.hip: pyramid_reduce_kernel) for one frame into a pitched
// output: one thread per output texel, four dword loads, the rounded mean of two channels at a time in 16-bit halves.
//
// motion_expand_kernel: one launch, one thread per output pixel; a wave is 64 pixels of one row, a workgroup 64 x 4 pixels.
// The workgroup covers 32 x 2 texels of mv_low and stages them plus a one-texel halo in LDS (34 x 4 halfwords), so each lane
// reads its nine neighbours -- mv_low at (x >> 1, y >> 1) + (a, b), a, b in {-1, 0, 1} -- from LDS.  A position outside mv_low
// gives no candidate; that is decided from the coordinates, so the halo's outside entries are never read as vectors.
//
// Step 1, the coarse neighbour: the doubled, saturated neighbours are the candidates.  Where all of a lane's candidates are
// equal the winner is that vector, with no cost work (on a pan: every lane).  Other lanes evaluate each DISTINCT candidate
// once against the (2R + 1)^2 curr window they keep in registers, as motion_refine.hip does.
// Step 2, the parity: the (2R + 3)^2 prev texels around q + w are read once and the nine costs of w + [-1, 1]^2 come from
// those registers.  A step that leaves [-127, 127] clamps back onto a vector that another step of the same nine gives, so it
// is left out instead of being evaluated twice.
//
// The cost, the key and the 64 x 4 launch are the window-cost family's (lfg_window_cost.hpp).  No atomics, no scratch, no
// data-dependent loop bounds.
#include "lfg_window_cost.hpp"

namespace lfg {
namespace {

constexpr int kExpTileW = kWinBlockX / 2 + 2, kExpTileH = kWinBlockY / 2 + 2;   // mv_low under the block, plus the halo
constexpr int kExpCands = 9;

__global__ __launch_bounds__(256) void frame_halve_kernel(const uint8_t *__restrict__ src, size_t srcPitch, int Ws, int Hs,
                                                          uint8_t *__restrict__ dst, size_t dstPitch, int Wd, int Hd) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)Wd * (size_t)Hd) return;
    const int y = (int)(i / (size_t)Wd), x = (int)(i - (size_t)y * (size_t)Wd);
    const int x0 = 2 * x, y0 = 2 * y, x1 = min(2 * x + 1, Ws - 1), y1 = min(2 * y + 1, Hs - 1);
    const uint32_t a = *reinterpret_cast<const uint32_t *>(src + (size_t)y0 * srcPitch + (size_t)x0 * 4u);
    const uint32_t b = *reinterpret_cast<const uint32_t *>(src + (size_t)y0 * srcPitch + (size_t)x1 * 4u);
    const uint32_t c = *reinterpret_cast<const uint32_t *>(src + (size_t)y1 * srcPitch + (size_t)x0 * 4u);
    const uint32_t d = *reinterpret_cast<const uint32_t *>(src + (size_t)y1 * srcPitch + (size_t)x1 * 4u);
    // channels 0 and 2 / 1 and 3 in 16-bit halves: four bytes plus 2 stay below 2^11
    const uint32_t even = (a & 0x00FF00FFu) + (b & 0x00FF00FFu) + (c & 0x00FF00FFu) + (d & 0x00FF00FFu) + 0x00020002u;
    const uint32_t odd = ((a >> 8) & 0x00FF00FFu) + ((b >> 8) & 0x00FF00FFu) + ((c >> 8) & 0x00FF00FFu) + ((d >> 8) & 0x00FF00FFu) + 0x00020002u;
    *reinterpret_cast<uint32_t *>(dst + (size_t)y * dstPitch + (size_t)x * 4u) = ((even >> 2) & 0x00FF00FFu) | (((odd >> 2) & 0x00FF00FFu) << 8);
}

// dbl(v) as an MV_S8X2 word
__device__ __forceinline__ uint32_t doubled_word(uint32_t word) {
    const Mv v = mv_unpack((uint16_t)word);
    return mv_word(clampi(2 * v.x, -127, 127), clampi(2 * v.y, -127, 127));
}

template <int R>
__global__ __launch_bounds__(kWinBlockX * kWinBlockY) void motion_expand_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mvLow, size_t mvLowPitch, uint8_t *__restrict__ mvOut, size_t mvOutPitch, int W, int H) {
    constexpr int D = 2 * R + 1, E = D + 2;
    __shared__ uint16_t tile[kExpTileH * kExpTileW];
    const int x0 = (int)blockIdx.x * kWinBlockX, y0 = (int)blockIdx.y * kWinBlockY;
    const int Wl = (W + 1) / 2, Hl = (H + 1) / 2;
    // one load per thread covers the tile: all of them are in flight before the first LDS write
    {
        const int i = (int)(threadIdx.y * kWinBlockX + threadIdx.x);
        const int gx = x0 / 2 - 1 + i % kExpTileW, gy = y0 / 2 - 1 + i / kExpTileW;
        const uint16_t staged = (i < kExpTileH * kExpTileW && gx >= 0 && gx < Wl && gy >= 0 && gy < Hl)
                                    ? *reinterpret_cast<const uint16_t *>(mvLow + (size_t)gy * mvLowPitch + (size_t)gx * 2u) : (uint16_t)0;
        if (i < kExpTileH * kExpTileW) tile[i] = staged;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= W || y >= H) return;

    const int nx0 = x >> 1, ny0 = y >> 1;
    const int t0 = (ny0 - y0 / 2 + 1) * kExpTileW + nx0 - x0 / 2 + 1;
    uint32_t cand[kExpCands];                                // k = 0 is the centre, then b, then a, skipping (0, 0)
    uint32_t present = 1u;                                   // bit k: neighbour k lies inside mv_low
    bool uniform = true;
    cand[0] = doubled_word(tile[t0]);
    {
        int k = 1;
#pragma unroll
        for (int b = -1; b <= 1; ++b)
#pragma unroll
            for (int a = -1; a <= 1; ++a) {
                if (a == 0 && b == 0) continue;
                cand[k] = doubled_word(tile[t0 + b * kExpTileW + a]);
                const int nx = nx0 + a, ny = ny0 + b;
                const bool in = nx >= 0 && nx < Wl && ny >= 0 && ny < Hl;
                present |= (in ? 1u : 0u) << k;
                uniform = uniform && (!in || cand[k] == cand[0]);
                ++k;
            }
    }

    // curr's window, read once; texels outside the image are skipped (bit clear in `inWin`)
    uint32_t cw[D * D];
    uint32_t inWin = 0u;
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int rx = x + i - R, ry = y + j - R;
            inWin |= (rx >= 0 && rx < W && ry >= 0 && ry < H ? 1u : 0u) << (j * D + i);
            cw[j * D + i] = texel_or_zero(curr, currPitch, rx, ry, W, H);
        }

    // step 1: the coarse neighbour
    Mv w = mv_unpack((uint16_t)cand[0]);
    if (!uniform) {
        uint64_t best = ~0ull;
#pragma unroll
        for (int k = 0; k < kExpCands; ++k) {
            bool fresh = (present >> k) & 1u;                // present and not equal to an earlier present candidate
#pragma unroll
            for (int m = 0; m < k; ++m) fresh = fresh && !(((present >> m) & 1u) && cand[m] == cand[k]);
            if (!fresh) continue;
            const Mv v = mv_unpack((uint16_t)cand[k]);
            uint32_t cost = 0u;
#pragma unroll
            for (int j = 0; j < D; ++j)
#pragma unroll
                for (int i = 0; i < D; ++i)
                    cost = window_add(cw, inWin, j * D + i, texel_or_zero(prev, prevPitch, x + i - R + v.x, y + j - R + v.y, W, H), cost);
            const uint64_t key = ((uint64_t)cost << 32) | mv_order_key(v.x, v.y);
            best = key < best ? key : best;
        }
        w = mv_order_decode((uint32_t)best);
    }

    // step 2: the parity.  pw[(j + 1) * E + (i + 1)] = prev at window texel (i, j) + w; a step (dx, dy) shifts the index.
    uint32_t pw[E * E];
#pragma unroll
    for (int j = 0; j < E; ++j)
#pragma unroll
        for (int i = 0; i < E; ++i) pw[j * E + i] = texel_or_zero(prev, prevPitch, x + i - R - 1 + w.x, y + j - R - 1 + w.y, W, H);
    uint64_t best = ~0ull;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            uint32_t cost = 0u;
#pragma unroll
            for (int j = 0; j < D; ++j)
#pragma unroll
                for (int i = 0; i < D; ++i) cost = window_add(cw, inWin, j * D + i, pw[(j + 1 + dy) * E + i + 1 + dx], cost);
            const int vx = w.x + dx, vy = w.y + dy;
            const bool inRange = vx >= -127 && vx <= 127 && vy >= -127 && vy <= 127;      // else: a duplicate of another step
            const uint64_t key = inRange ? ((uint64_t)cost << 32) | mv_order_key(vx, vy) : ~0ull;
            best = key < best ? key : best;
        }
    const Mv v = mv_order_decode((uint32_t)best);
    *reinterpret_cast<uint16_t *>(mvOut + (size_t)y * mvOutPitch + (size_t)x * 2u) = mv_word(v.x, v.y);
}

}  // namespace

hipError_t launch_frame_halve(hipStream_t s, const lfg_frame &in, const lfg_frame &out) {
    const size_t n = (size_t)out.width * out.height;
    hipLaunchKernelGGL(frame_halve_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, (const uint8_t *)in.data, (size_t)in.pitch,
                       (int)in.width, (int)in.height, (uint8_t *)out.data, (size_t)out.pitch, (int)out.width, (int)out.height);
    return hipGetLastError();
}

hipError_t launch_motion_expand(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvLow,
                                const lfg_frame &mvOut, int radius) {
    return window_cost_launch(motion_expand_kernel<0>, motion_expand_kernel<1>, motion_expand_kernel<2>, radius, s, prev, curr, mvLow, mvOut);
}

}  // namespace lfg
