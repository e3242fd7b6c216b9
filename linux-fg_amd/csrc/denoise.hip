// denoise.hip -- motion-compensated temporal denoising (lfg_denoise_temporal, include/linuxfg_hip.h).  No reference counterpart;
// opt-in, in the caller's loop, in front of everything that thresholds per-pixel differences.  tests/denoise_model.py restates
// the definition on the CPU, and lfg_denoise.hpp holds the per-pixel arithmetic that the kernel shares with the CPU check
// (tests/cpp/denoise_on_host.cpp).
//
// One launch, one thread per output pixel; a wave is 64 pixels of one row, a workgroup 64 x 4 pixels (the window-cost family's
// shape, lfg_window_cost.hpp).  A lane reads its vector of each reference (2 bytes), keeps the (2R + 1)^2 curr window in
// registers, gathers the same window of each reference displaced by that reference's vector -- every load of every reference
// in flight before the first use of any -- and sums the window cost per reference with v_sad_u8.  The centre texel of a
// gathered window is the texel the pixel is mixed with: no further load.  Weights, shares, mix and limit are lfg_denoise.hpp's.
// Instantiated by radius (0, 1, 2) and by the number of references (1, 2): the window and the references are unrolled.
//
// No LDS, no cross-lane operation, no atomics and no data-dependent branch: the cost does not depend on the content, and a
// reference that is refused (weight 0) costs what an accepted one does.  Integers only; the two divisions per pixel are plain
// unsigned 32-bit divisions.  Byte offsets are size_t throughout.
//
// Traffic per pixel: 4 bytes of curr and 4 written, plus per reference 2 bytes of vectors and 4 bytes of the reference where the
// field is smooth; the other (2R + 1)^2 - 1 texels of each window are the neighbouring lanes' own and come from the caches
// (DESIGN.md section 4.27).
#include "lfg_denoise.hpp"
#include "lfg_window_cost.hpp"

namespace lfg {
namespace {

struct DenoiseRef { const uint8_t *img; size_t pitch; const uint8_t *mv; size_t mvPitch; };

template <int R, int N>
__global__ __launch_bounds__(kWinBlockX * kWinBlockY) void denoise_temporal_kernel(
        const uint8_t *__restrict__ curr, size_t currPitch, DenoiseRef ref0, DenoiseRef ref1, uint8_t *__restrict__ out,
        size_t outPitch, int W, int H, uint32_t tolerance, uint32_t strength, uint32_t limit) {
    constexpr int D = 2 * R + 1, kCentre = R * D + R;
    const int x = (int)blockIdx.x * kWinBlockX + (int)threadIdx.x, y = (int)blockIdx.y * kWinBlockY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const DenoiseRef refs[kDenoiseMaxRefs] = {ref0, ref1};

    Mv v[N];
#pragma unroll
    for (int i = 0; i < N; ++i)
        v[i] = mv_unpack(*reinterpret_cast<const uint16_t *>(refs[i].mv + (size_t)y * refs[i].mvPitch + (size_t)x * 2u));

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

    // every gathered load of every reference, before the first use of any
    uint32_t rw[N][D * D];
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int i = 0; i < D; ++i)
                rw[k][j * D + i] = texel_or_zero(refs[k].img, refs[k].pitch, x + i - R + v[k].x, y + j - R + v[k].y, W, H);

    const uint32_t L = tolerance * (uint32_t)__builtin_popcount(inWin);
    uint32_t w[kDenoiseMaxRefs] = {0u, 0u};
#pragma unroll
    for (int k = 0; k < N; ++k) {
        uint32_t cost = 0u;
#pragma unroll
        for (int t = 0; t < D * D; ++t) cost = window_add(cw, inWin, t, rw[k][t], cost);
        const int tx = x + v[k].x, ty = y + v[k].y;
        w[k] = denoise_weight(strength, L, cost, tx >= 0 && tx < W && ty >= 0 && ty < H);
    }
    const DenoiseShares s = denoise_shares(L, w[0], w[1]);
    const uint32_t px = denoise_texel(s, cw[kCentre], rw[0][kCentre], N > 1 ? rw[N - 1][kCentre] : 0u, limit);
    *reinterpret_cast<uint32_t *>(out + (size_t)y * outPitch + (size_t)x * 4u) = px;
}

template <int N>
auto denoise_kernel_for(int radius) {
    return radius == 0 ? denoise_temporal_kernel<0, N> : radius == 1 ? denoise_temporal_kernel<1, N> : denoise_temporal_kernel<2, N>;
}

}  // namespace

hipError_t launch_denoise_temporal(hipStream_t s, const lfg_frame &curr, const lfg_frame *const *refs, const lfg_frame *const *mvs,
                                   int count, const lfg_frame &out, int radius, int tolerance, int strength, int limit) {
    const int W = (int)curr.width, H = (int)curr.height;
    DenoiseRef r[kDenoiseMaxRefs];
    for (int i = 0; i < kDenoiseMaxRefs; ++i) {
        const int k = i < count ? i : 0;                     // (an absent second reference is never read)
        r[i] = DenoiseRef{(const uint8_t *)refs[k]->data, (size_t)refs[k]->pitch, (const uint8_t *)mvs[k]->data, (size_t)mvs[k]->pitch};
    }
    const dim3 block(kWinBlockX, kWinBlockY), grid((unsigned)((W + kWinBlockX - 1) / kWinBlockX), (unsigned)((H + kWinBlockY - 1) / kWinBlockY));
    hipLaunchKernelGGL(count == 1 ? denoise_kernel_for<1>(radius) : denoise_kernel_for<2>(radius), grid, block, 0, s,
                       (const uint8_t *)curr.data, (size_t)curr.pitch, r[0], r[1], (uint8_t *)out.data, (size_t)out.pitch, W, H,
                       (uint32_t)tolerance, (uint32_t)strength, (uint32_t)limit);
    return hipGetLastError();
}

}  // namespace lfg
