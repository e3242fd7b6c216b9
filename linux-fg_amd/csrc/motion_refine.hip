// motion_refine.hip -- per-pixel vector refinement (lfg_motion_refine, include/linuxfg_hip.h).  No reference counterpart; opt-in,
// between either estimator and either interpolator.  tests/refine_model.c restates the definition on the CPU.
//
// One launch, one thread per output pixel; a wave is 64 pixels of one row, a workgroup 64 x 4 pixels.  The workgroup stages
// mv_in of its tile plus an 8-pixel halo in LDS (80 x 20 halfwords, 3.2 KB), so each lane reads its 17 candidates -- mv_in at
// q and at q + (a s, b s), a, b in {-1, 0, 1}, s in {4, 8} -- from LDS.  A candidate position outside the image gives no
// candidate; that is decided from the coordinates, so the halo's outside entries are never read as vectors.
//
// Uniform lanes: when every candidate equals mv_in(q) the answer is mv_in(q) (the definition's minimum over one distinct
// vector), stored without any cost work.  On a pan that is every lane away from the image's own edges.
//
// Other lanes keep the (2R + 1)^2 curr window in registers (read once), then evaluate each DISTINCT candidate once by the
// family's rule (lfg_window_cost.hpp: the cost, the key, the 64 x 4 launch).  No atomics, no second launch.
//
// Traffic per pixel: 2 bytes of mv_in (plus the halo, L2 hits) and 2 of mv_out on a uniform lane; a non-uniform lane adds
// (2R + 1)^2 dwords of curr and up to 17 (2R + 1)^2 gathered dwords of prev, mostly L1/L2 hits.
#include "lfg_window_cost.hpp"

namespace lfg {
namespace {

constexpr int kRefHalo = 8;                                  // the farthest candidate offset
constexpr int kRefTileW = kWinBlockX + 2 * kRefHalo, kRefTileH = kWinBlockY + 2 * kRefHalo;
constexpr int kRefCands = 17;

// Candidate k's offset: k = 0 is (0, 0); k = 1 .. 16 run over s = 4, 8, then b, then a, skipping (a, b) = (0, 0).
__device__ constexpr int kRefDx[kRefCands] = {0, -4, 0, 4, -4, 4, -4, 0, 4, -8, 0, 8, -8, 8, -8, 0, 8};
__device__ constexpr int kRefDy[kRefCands] = {0, -4, -4, -4, 0, 0, 4, 4, 4, -8, -8, -8, 0, 0, 8, 8, 8};

template <int R>
__global__ __launch_bounds__(kWinBlockX * kWinBlockY) void motion_refine_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mvIn, size_t mvInPitch, uint8_t *__restrict__ mvOut, size_t mvOutPitch, int W, int H) {
    constexpr int D = 2 * R + 1;
    __shared__ uint16_t tile[kRefTileH * kRefTileW];
    const int x0 = (int)blockIdx.x * kWinBlockX, y0 = (int)blockIdx.y * kWinBlockY;
    // every load of the tile in flight before the first LDS write: a loop that waits for each load in turn is latency-bound
    constexpr int kThreads = kWinBlockX * kWinBlockY, kSteps = (kRefTileH * kRefTileW + kThreads - 1) / kThreads;
    uint16_t staged[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        const int i = (int)(threadIdx.y * kWinBlockX + threadIdx.x) + k * kThreads;
        const int gx = x0 - kRefHalo + i % kRefTileW, gy = y0 - kRefHalo + i / kRefTileW;
        staged[k] = (i < kRefTileH * kRefTileW && gx >= 0 && gx < W && gy >= 0 && gy < H)
                        ? *reinterpret_cast<const uint16_t *>(mvIn + (size_t)gy * mvInPitch + (size_t)gx * 2u) : (uint16_t)0;
    }
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        const int i = (int)(threadIdx.y * kWinBlockX + threadIdx.x) + k * kThreads;
        if (i < kRefTileH * kRefTileW) tile[i] = staged[k];
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = y0 + (int)threadIdx.y;
    if (x >= W || y >= H) return;

    const int t0 = ((int)threadIdx.y + kRefHalo) * kRefTileW + (int)threadIdx.x + kRefHalo;
    uint32_t cand[kRefCands];
    uint32_t present = 1u;                                   // bit k: candidate k's position is inside the image
    bool uniform = true;
#pragma unroll
    for (int k = 0; k < kRefCands; ++k) {
        cand[k] = tile[t0 + kRefDy[k] * kRefTileW + kRefDx[k]];
        if (k == 0) continue;
        const int nx = x + kRefDx[k], ny = y + kRefDy[k];
        const bool in = nx >= 0 && nx < W && ny >= 0 && ny < H;
        present |= (in ? 1u : 0u) << k;
        uniform = uniform && (!in || cand[k] == cand[0]);
    }
    uint16_t *dst = reinterpret_cast<uint16_t *>(mvOut + (size_t)y * mvOutPitch + (size_t)x * 2u);
    if (uniform) {
        *dst = (uint16_t)cand[0];
        return;
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

    uint64_t best = ~0ull;
#pragma unroll
    for (int k = 0; k < kRefCands; ++k) {
        bool fresh = (present >> k) & 1u;                    // present and not equal to an earlier present candidate
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
    const Mv v = mv_order_decode((uint32_t)best);
    *dst = mv_word(v.x, v.y);
}

}  // namespace

hipError_t launch_motion_refine(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvIn,
                                const lfg_frame &mvOut, int radius) {
    return window_cost_launch(motion_refine_kernel<0>, motion_refine_kernel<1>, motion_refine_kernel<2>, radius, s, prev, curr, mvIn, mvOut);
}

}  // namespace lfg
