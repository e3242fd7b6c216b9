// interpolate_bicubic.hip -- the compensated routes' sampling step with the bicubic fetch (lfg_interpolate_compensated_sampled with
// LFG_SAMPLING_BICUBIC, include/linuxfg_hip.h).  No reference counterpart; opt-in.  tests/bicubic_model.c
// restates every step on the CPU.
//
// The projection is interpolate_mc.hip's or interpolate_subpel.hip's, launched as it is; what follows it here is
//   mc_bicubic_kernel   the sibling of mc_interpolate_kernel (MV_S8X2 vectors, 32-bit keys),
//   mcq_bicubic_kernel  the sibling of mcq_sample_kernel (MV_S16X2_Q2 vectors, 64-bit keys):
// one thread per output pixel, K, the hole walk where K is a hole, both fetches, the hole rule, the blend.  K, the walks, the
// gate reads and the end of a pixel are lfg_mc.hpp's, the taps lfg_interp.hpp's, the weights and the integer body
// lfg_bicubic.hpp's.  A weight row is computed from its phase, a dozen integer operations per fetch and axis, not read from a
// table in LDS: no staging, no barrier, and phase 64 (a fraction that rounds to 1.0f) needs no 65th row.
//
// Loads: 16 dwords per fetch from clamped addresses, both fetches' issued before either is used.  Wave-uniform shortcuts, legal
// because a phase of 0 weighs its axis (0, 16384, 0, 0) and the integer body then returns 256 * texel exactly: where the vertical
// phase of both fetches is 0 on every lane of the wave only row 1 is loaded, likewise column 1, and where both hold the fetch is
// the single texel and skips the integer body.  An integer pan with even vectors at t = 0.5 takes that last path everywhere.
//
// Traffic per pixel and factor: the projection's, then K + 128 (two fetches of 16 texels, all but a few cached neighbours) + 4
// (out); 8 + 4 on the single-texel path.
#include "lfg_mc.hpp"

namespace lfg {

namespace {

// Both fetches of a pixel from their positions, and its end.  hole_only() is evaluated after the loads are issued and gives the
// hole rule's verdict (lfg_mc.hpp: mc_store_inside_or_blend's `only`).
template <typename HoleRule>
__device__ __forceinline__ void bicubic_pixel(const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr,
                                              int currPitch, int W, int H, float Px, float Py, float Cx, float Cy, float t,
                                              uint8_t *__restrict__ out, size_t outPitch, int x, int y, HoleRule hole_only) {
    const BicubicTaps sp = bicubic_taps(prev, W, H, prevPitch, Px, Py);
    const BicubicTaps sc = bicubic_taps(curr, W, H, currPitch, Cx, Cy);
    // wave-uniform: does any lane have a horizontal / a vertical fraction?
    const bool allCols = __builtin_amdgcn_ballot_w64((sp.phiX | sc.phiX) != 0) != 0ull;
    const bool allRows = __builtin_amdgcn_ballot_w64((sp.phiY | sc.phiY) != 0) != 0ull;
    const BicubicTexels tp = bicubic_load(sp, allRows, allCols), tc = bicubic_load(sc, allRows, allCols);   // both fetches in flight
    const int only = hole_only();
    V4 P, C;
    if (!allRows && !allCols) {
        P = unorm4(tp.t[5]); C = unorm4(tc.t[5]);
    } else {
        P = bicubic_value(sp, tp); C = bicubic_value(sc, tc);
    }
    mc_store_inside_or_blend_values(P, sp.inside, C, sc.inside, only, t, out, outPitch, x, y);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_bicubic_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint32_t *__restrict__ keys, int W, int H, float t, int matchSad,
        uint8_t *__restrict__ out, size_t outPitch) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const float s = 1.0f - t;
    uint32_t key = keys[(size_t)y * (size_t)W + (size_t)x];
    const bool hole = key == kMcHole;
    if (hole) key = mc_fill_vector<false>(keys, W, H, x, y);
    const Mv u = mv_order_decode(key);
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float Px = px + (float)u.x * t, Py = py + (float)u.y * t;
    const float Cx = px - (float)u.x * s, Cy = py - (float)u.y * s;
    bicubic_pixel(prev, prevPitch, curr, currPitch, W, H, Px, Py, Cx, Cy, t, out, outPitch, x, y, [&]() {
        // 0: blend as a projected pixel, 1: prev's sample alone (covered), 2: curr's alone (revealed)
        if (!hole) return 0;
        const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
        const Mv vc = mv_at(mv, mvPitch, cx, cy);
        if (!matched(prev, (size_t)prevPitch, texel_u32(curr, (size_t)currPitch, cx, cy), W, H, cx, cy, vc, matchSad)) return 2;
        return vc.x != u.x || vc.y != u.y ? 1 : 0;
    });
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mcq_bicubic_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mvq, size_t mvqPitch, const unsigned long long *__restrict__ keys, int W, int H, float t, int matchSad,
        uint8_t *__restrict__ out, size_t outPitch) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const float s = 1.0f - t;
    unsigned long long key = keys[(size_t)y * (size_t)W + (size_t)x];
    const bool hole = key == kMcqHole;
    if (hole) key = mcq_fill_vector(keys, W, H, x, y);
    const Mv u = mvq_order_decode(key);
    const float ux = (float)u.x * 0.25f, uy = (float)u.y * 0.25f;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float Px = px + ux * t, Py = py + uy * t;
    const float Cx = px - ux * s, Cy = py - uy * s;
    bicubic_pixel(prev, prevPitch, curr, currPitch, W, H, Px, Py, Cx, Cy, t, out, outPitch, x, y, [&]() {
        if (!hole) return 0;
        const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
        const Mv wc = mvq_at(mvq, mvqPitch, cx, cy);
        if (!matched_q(prev, (size_t)prevPitch, texel_u32(curr, (size_t)currPitch, cx, cy), W, H, cx, cy, wc, matchSad)) return 2;
        return wc.x != u.x || wc.y != u.y ? 1 : 0;
    });
}

}  // namespace

// Clear K and project as the bilinear routes do, then the bicubic sampling kernel of that route.
hipError_t launch_interpolate_compensated_bicubic(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                                  const lfg_frame &out, float factor, int matchSad, uint32_t *keys) {
    const int W = (int)curr.width, H = (int)curr.height;
    hipError_t e = launch_compensated_projection(s, prev, curr, mv, factor, matchSad, keys);
    if (e == hipSuccess)
        e = mc_launch(mc_bicubic_kernel, mc_grid(W, H), s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (const uint32_t *)keys, W, H, factor, matchSad,
                      (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

hipError_t launch_interpolate_compensated_subpel_bicubic(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr,
                                                         const lfg_frame &mvq, const lfg_frame &out, float factor, int matchSad,
                                                         unsigned long long *keys) {
    const int W = (int)curr.width, H = (int)curr.height;
    hipError_t e = launch_compensated_projection_subpel(s, prev, curr, mvq, factor, matchSad, keys);
    if (e == hipSuccess)
        e = mc_launch(mcq_bicubic_kernel, mc_grid(W, H), s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)mvq.data, (size_t)mvq.pitch, (const unsigned long long *)keys, W, H, factor,
                      matchSad, (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

}  // namespace lfg
