// interpolate_subpel.hip -- motion-compensated interpolation along quarter-pixel vectors (lfg_interpolate_compensated_subpel,
// include/linuxfg_hip.h): interpolate_mc.hip's definition with a fractional gate, a projection that carries the fraction, and
// a key image of 64-bit words.  No reference counterpart; opt-in.  tests/subpel_model.c restates every step on the CPU.
//
// Two launches per factor, after the key image K (W * H 64-bit words, the lane's scratch of this route) has been set to 0xFF
// bytes in stream order:
//   mcq_project_kernel  one thread per source pixel q: the fractional gate (four texels of prev), then one atomicMin of the
//                       vector's 64-bit key into K(q + d) -- a single global_atomic_umin_x2, no compare-and-swap loop;
//   mcq_sample_kernel   one thread per output pixel: K, the hole walk where K is a hole, both bilinear fetches, the blend.
// The second launch never writes K.  The gate (matched_q), the walk (mcq_fill_vector) and the end of a pixel
// (mc_store_inside_or_blend) are lfg_mc.hpp's; the word, the key and its decode are lfg_vector_word.hpp's; the taps are
// lfg_interp.hpp's.  With mvq = 4 * mv every step computes what interpolate_mc.hip computes from mv: the gate's weights are
// (16, 0, 0, 0), (float)(4 v) * 0.25f is (float)v exactly, and 16 |v|^2 orders as |v|^2 does.
//
// Traffic per pixel and factor: 8 (clear) + 4 (mvq) + 4 (curr) + 16 (gathered prev, mostly cached neighbours) + 8 (atomic) in
// the projection, 8 (K) + 8 (two fetches) + 4 (out) in the sampling.
// Not built: masked, bidirectional, extrapolating and fill-plane variants.
#include "lfg_mc.hpp"

namespace lfg {

namespace {

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mcq_project_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mvq, size_t mvqPitch, int W, int H, float t, int matchSad, unsigned long long *__restrict__ keys) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const Mv w = mvq_at(mvq, mvqPitch, x, y);
    const uint32_t c = texel_u32(curr, currPitch, x, y);
    if (!matched_q(prev, prevPitch, c, W, H, x, y, w, matchSad)) return;
    const float s = 1.0f - t;
    const int dx = x + (int)__builtin_floorf(((float)w.x * 0.25f) * s + 0.5f), dy = y + (int)__builtin_floorf(((float)w.y * 0.25f) * s + 0.5f);
    if (dx < 0 || dx >= W || dy < 0 || dy >= H) return;
    atomicMin(keys + (size_t)dy * (size_t)W + (size_t)dx, (unsigned long long)mvq_longest_first_key(w.x, w.y));   // result unused
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mcq_sample_kernel(
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
    const SampleTaps sp = pixel_taps(prev, W, H, prevPitch, Px, Py);
    const SampleTaps sc = pixel_taps(curr, W, H, currPitch, Cx, Cy);
    const SampleTexels tp = sample_load(sp), tc = sample_load(sc);        // both fetches in flight before either is used
    // 0: blend as a projected pixel, 1: prev's sample alone (covered), 2: curr's alone (revealed)
    int only = 0;
    if (hole) {
        const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
        const Mv wc = mvq_at(mvq, mvqPitch, cx, cy);
        if (!matched_q(prev, (size_t)prevPitch, texel_u32(curr, (size_t)currPitch, cx, cy), W, H, cx, cy, wc, matchSad)) only = 2;
        else if (wc.x != u.x || wc.y != u.y) only = 1;
    }
    mc_store_inside_or_blend(sp, tp, sc, tc, only, t, out, outPitch, x, y);
}

}  // namespace

// Clear K, project: on its own for a sampling kernel of another file (interpolate_bicubic.hip).
hipError_t launch_compensated_projection_subpel(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvq,
                                                float factor, int matchSad, unsigned long long *keys) {
    const int W = (int)curr.width, H = (int)curr.height;
    hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)W * (size_t)H * 8u, s);
    if (e == hipSuccess)
        e = mc_launch(mcq_project_kernel, mc_grid(W, H), s, (const uint8_t *)prev.data, (size_t)prev.pitch, (const uint8_t *)curr.data,
                      (size_t)curr.pitch, (const uint8_t *)mvq.data, (size_t)mvq.pitch, W, H, factor, matchSad, keys);
    return e;
}

// Clear K, project, sample.
hipError_t launch_interpolate_compensated_subpel(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvq,
                                                 const lfg_frame &out, float factor, int matchSad, unsigned long long *keys) {
    const int W = (int)curr.width, H = (int)curr.height;
    const dim3 grid = mc_grid(W, H);
    hipError_t e = launch_compensated_projection_subpel(s, prev, curr, mvq, factor, matchSad, keys);
    if (e == hipSuccess)
        e = mc_launch(mcq_sample_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)mvq.data, (size_t)mvq.pitch, (const unsigned long long *)keys, W, H, factor,
                      matchSad, (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

}  // namespace lfg
