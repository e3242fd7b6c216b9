// interpolate_bidir.hip -- bidirectional motion-compensated interpolation (lfg_interpolate_compensated_bidirectional,
// include/linuxfg_hip.h) and the forward-backward check on its own (lfg_motion_consistency).  No reference counterpart;
// opt-in, next to interpolate_mc.hip, whose definition it keeps but for three things: a vector projects only when the field
// measured the other way confirms it, prev's grid projects too, and a hole's revealed / covered decision asks both frames.
// The predicates are lfg_mc_bidir.hpp's; the hole word, the reads, the match gate, the hole walk (mc_fill_vector), the end of
// a pixel (mc_store_inside_or_blend) and the launchers' steps lfg_mc.hpp's, the same functions interpolate_mc.hip calls; the
// key, its decode and the hole walk's order lfg_vector_word.hpp's; the taps lfg_interp.hpp's.  tests/bidir_model.c restates
// every step below on the CPU.
//
// Three launches per factor, after the key image K (W * H words, the lane's scratch, interpolate_mc.hip's) has been set to
// 0xFF bytes in stream order:
//   bidir_project_kernel<false>  one thread per pixel q of curr's grid: confirmed_f, then one atomicMin of f's key into
//                                K(q + floor(f s + 0.5));
//   bidir_project_kernel<true>   one thread per pixel p of prev's grid: confirmed_b, then one atomicMin of (-b)'s key into
//                                K(p + floor(b t + 0.5)).  The key order is total and atomicMin commutes: the two launches
//                                give the same K in either order;
//   bidir_sample_kernel          one thread per output pixel: K, the hole walk where K is a hole, both bilinear fetches, the
//                                symmetric hole rule, the blend.  It never writes K.
// Under lfg_set_hole_reach hole_fill.hip's two passes run before the third launch, which is then bidir_sample_plane_kernel: the
// same body with one load of the fill plane where the walk was.
//
// Traffic per pixel and factor: 4 (clear) + 2 x (2 (own vector) + 4 (own texel) + 4 (gathered far texel) + 2 (gathered other
// vector) + 4 (atomic)) in the projections, 4 (K) + 8 (two fetches, mostly cached neighbours) + 4 (out) in the sampling:
// 52 bytes, 431 MB at 4K, against interpolate_mc.hip's 34.
#include "lfg_mc_bidir.hpp"

namespace lfg {

namespace {

// Forward: own = curr, far = prev, mine = fwd, other = bwd.  Backward: own = prev, far = curr, mine = bwd, other = fwd.
template <bool Backward>
__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void bidir_project_kernel(
        const uint8_t *__restrict__ own, size_t ownPitch, const uint8_t *__restrict__ far, size_t farPitch,
        const uint8_t *__restrict__ mine, size_t minePitch, const uint8_t *__restrict__ other, size_t otherPitch, int W, int H,
        float t, int matchSad, int tolerance, uint32_t *__restrict__ keys) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const Mv a = mv_at(mine, minePitch, x, y);
    const uint32_t texel = texel_u32(own, ownPitch, x, y);
    if (!bidir_confirmed<Backward>(far, farPitch, texel, other, otherPitch, W, H, x, y, a, matchSad, tolerance)) return;
    const float scale = Backward ? t : 1.0f - t;
    const int dx = x + (int)__builtin_floorf((float)a.x * scale + 0.5f), dy = y + (int)__builtin_floorf((float)a.y * scale + 0.5f);
    if (dx < 0 || dx >= W || dy < 0 || dy >= H) return;
    // the content of p moves by +b per interval: in fwd's convention it carries -b
    const uint32_t key = Backward ? mv_longest_first_key(-a.x, -a.y) : mv_longest_first_key(a.x, a.y);
    atomicMin(keys + (size_t)dy * (size_t)W + (size_t)dx, key);       // result unused: one global_atomic_umin
}

// Plane: a hole takes its vector from the fill plane `fill` (hole_fill.hip), one load, instead of walking K.
template <bool Plane>
__device__ __forceinline__ void bidir_sample(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ fwd, size_t fwdPitch, const uint8_t *__restrict__ bwd, size_t bwdPitch,
        const uint32_t *__restrict__ keys, const uint32_t *__restrict__ fill, int W, int H, float t, int matchSad, int tolerance,
        uint8_t *__restrict__ out, size_t outPitch) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const float s = 1.0f - t;
    uint32_t key = keys[(size_t)y * (size_t)W + (size_t)x];
    const bool hole = key == kMcHole;
    if (hole) key = Plane ? mc_fill_from_plane(fill, W, x, y) : mc_fill_vector<false>(keys, W, H, x, y);
    const Mv u = mv_order_decode(key);
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float Px = px + (float)u.x * t, Py = py + (float)u.y * t;
    const float Cx = px - (float)u.x * s, Cy = py - (float)u.y * s;
    const SampleTaps sp = pixel_taps(prev, W, H, prevPitch, Px, Py);
    const SampleTaps sc = pixel_taps(curr, W, H, currPitch, Cx, Cy);
    const SampleTexels tp = sample_load(sp), tc = sample_load(sc);        // both fetches in flight before either is used
    // 0: blend as a projected pixel, 1: prev's sample alone (covered in curr), 2: curr's alone (revealed in curr)
    int only = 0;
    if (hole) {
        const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
        const int qx = clampi((int)__builtin_floorf(Px), 0, W - 1), qy = clampi((int)__builtin_floorf(Py), 0, H - 1);
        const Mv fc = mv_at(fwd, fwdPitch, cx, cy), bp = mv_at(bwd, bwdPitch, qx, qy);
        const uint32_t cTexel = texel_u32(curr, (size_t)currPitch, cx, cy), pTexel = texel_u32(prev, (size_t)prevPitch, qx, qy);
        // curr / prev shows other, confirmed content there
        const bool cBad = (fc.x != u.x || fc.y != u.y) &&
                          bidir_confirmed<false>(prev, (size_t)prevPitch, cTexel, bwd, bwdPitch, W, H, cx, cy, fc, matchSad, tolerance);
        const bool pBad = (-bp.x != u.x || -bp.y != u.y) &&
                          bidir_confirmed<true>(curr, (size_t)currPitch, pTexel, fwd, fwdPitch, W, H, qx, qy, bp, matchSad, tolerance);
        only = cBad && !pBad ? 1 : (pBad && !cBad ? 2 : 0);
    }
    mc_store_inside_or_blend(sp, tp, sc, tc, only, t, out, outPitch, x, y);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void bidir_sample_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ fwd, size_t fwdPitch, const uint8_t *__restrict__ bwd, size_t bwdPitch,
        const uint32_t *__restrict__ keys, int W, int H, float t, int matchSad, int tolerance, uint8_t *__restrict__ out,
        size_t outPitch) {
    bidir_sample<false>(prev, prevPitch, curr, currPitch, fwd, fwdPitch, bwd, bwdPitch, keys, nullptr, W, H, t, matchSad, tolerance, out,
                        outPitch);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void bidir_sample_plane_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ fwd, size_t fwdPitch, const uint8_t *__restrict__ bwd, size_t bwdPitch,
        const uint32_t *__restrict__ keys, const uint32_t *__restrict__ fill, int W, int H, float t, int matchSad, int tolerance,
        uint8_t *__restrict__ out, size_t outPitch) {
    bidir_sample<true>(prev, prevPitch, curr, currPitch, fwd, fwdPitch, bwd, bwdPitch, keys, fill, W, H, t, matchSad, tolerance, out,
                       outPitch);
}

// out(q) = 255 where a(q) is consistent with b, 0 elsewhere: one byte per thread, the W bytes of each row and no more.
__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void motion_consistency_kernel(
        const uint8_t *__restrict__ a, size_t aPitch, const uint8_t *__restrict__ b, size_t bPitch, int W, int H, int tolerance,
        uint8_t *__restrict__ mask, size_t maskPitch) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    mask[(size_t)y * maskPitch + (size_t)x] = bidir_consistent(b, bPitch, W, H, x, y, mv_at(a, aPitch, x, y), tolerance) ? 0xffu : 0u;
}

}  // namespace

// Clear K, project forward, project backward, sample.  With `fill` (lfg_set_hole_reach): the fill plane of `reach` into `fill`
// (W * H words, hole_fill.hip) before the sampling, and the kernel that reads it at holes.
hipError_t launch_interpolate_compensated_bidirectional(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &fwd,
                                                        const lfg_frame &bwd, const lfg_frame &out, float factor, int matchSad,
                                                        int tolerance, uint32_t *keys, uint32_t *fill, int reach) {
    const int W = (int)curr.width, H = (int)curr.height;
    dim3 grid;
    hipError_t e = mc_clear_keys(s, keys, W, H, grid);
    if (e == hipSuccess)
        e = mc_launch(bidir_project_kernel<false>, grid, s, (const uint8_t *)curr.data, (size_t)curr.pitch, (const uint8_t *)prev.data,
                      (size_t)prev.pitch, (const uint8_t *)fwd.data, (size_t)fwd.pitch, (const uint8_t *)bwd.data, (size_t)bwd.pitch,
                      W, H, factor, matchSad, tolerance, keys);
    if (e == hipSuccess)
        e = mc_launch(bidir_project_kernel<true>, grid, s, (const uint8_t *)prev.data, (size_t)prev.pitch, (const uint8_t *)curr.data,
                      (size_t)curr.pitch, (const uint8_t *)bwd.data, (size_t)bwd.pitch, (const uint8_t *)fwd.data, (size_t)fwd.pitch,
                      W, H, factor, matchSad, tolerance, keys);
    if (e == hipSuccess && fill) {
        e = launch_hole_fill_plane(s, keys, (size_t)W, fill, (size_t)W, W, H, reach, false);
        if (e == hipSuccess)
            e = mc_launch(bidir_sample_plane_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                          (int)curr.pitch, (const uint8_t *)fwd.data, (size_t)fwd.pitch, (const uint8_t *)bwd.data, (size_t)bwd.pitch,
                          (const uint32_t *)keys, (const uint32_t *)fill, W, H, factor, matchSad, tolerance, (uint8_t *)out.data,
                          (size_t)out.pitch);
        return e;
    }
    if (e == hipSuccess)
        e = mc_launch(bidir_sample_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)fwd.data, (size_t)fwd.pitch, (const uint8_t *)bwd.data, (size_t)bwd.pitch,
                      (const uint32_t *)keys, W, H, factor, matchSad, tolerance, (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

hipError_t launch_motion_consistency(hipStream_t s, const lfg_frame &a, const lfg_frame &b, int tolerance, const lfg_mask &out) {
    const int W = (int)a.width, H = (int)a.height;
    return mc_launch(motion_consistency_kernel, mc_grid(W, H), s, (const uint8_t *)a.data, (size_t)a.pitch, (const uint8_t *)b.data,
                     (size_t)b.pitch, W, H, tolerance, (uint8_t *)out.data, (size_t)out.pitch);
}

}  // namespace lfg
