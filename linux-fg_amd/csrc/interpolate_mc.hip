// interpolate_mc.hip -- motion-compensated interpolation (lfg_interpolate_compensated, include/linuxfg_hip.h): the vectors are
// projected forward to time t, then both frames are fetched along the projected vectors.  No reference counterpart; opt-in,
// next to interpolate.hip (the shader's path).  tests/mc_model.c restates every step below on the CPU.
//
// Two launches per factor, after the key image K (W * H words, the lane's scratch) has been set to 0xFF bytes in stream order:
//   mc_project_kernel      one thread per source pixel q: the match gate, then one atomicMin of the vector's key into K(q + d);
//   mc_interpolate_kernel  one thread per output pixel: K, the hole walk where K is a hole, both bilinear fetches, the blend.
// The second launch starts once every projection is visible, and it never writes K: a hole's walk reads words of its
// neighbours that other workgroups also read.  lfg_interpolate_compensated_masked runs the same two launches through
// mc_project_masked_kernel and mc_interpolate_masked_kernel (tests/overlay_model.c).  The project pair is one body,
// mc_project<Masked>, under two wrappers that keep the kernels' names and argument lists; the interpolate pair is two kernels
// that share their hole walk and the end of a pixel (see there).  The hole and static words, the reads, the match gate, the
// walk (mc_fill_vector), the end of a pixel (mc_store_inside_or_blend) and the launchers' steps are lfg_mc.hpp's, shared with
// extrapolate_mc.hip and interpolate_bidir.hip; the key, its decode and the hole walk's order are lfg_vector_word.hpp's.
// Under lfg_set_hole_reach the launchers put hole_fill.hip's two passes between the launches and run mc_interpolate_plane_kernel
// or mc_interpolate_masked_plane_kernel: the same bodies with one load of the fill plane where the walk was.
//
// Traffic per pixel and factor: 4 (clear) + 2 (mv) + 4 (curr) + 4 (gathered prev) + 4 (atomic) in the projection, 4 (K) + 8
// (two fetches, mostly cached neighbours) + 4 (out) in the interpolation: 34 bytes, 280 MB at 4K.
#include "lfg_mc.hpp"

namespace lfg {

namespace {

// Both project kernels.  Masked: one more byte of traffic per pixel, and a static pixel projects its own vector as any other.
template <bool Masked>
__device__ __forceinline__ void mc_project(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint8_t *__restrict__ mask, size_t maskPitch, int W, int H, float t,
        int matchSad, uint32_t *__restrict__ keys) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    uint8_t isStatic = 0;
    if constexpr (Masked) isStatic = mask[(size_t)y * maskPitch + (size_t)x];
    const Mv v = mv_at(mv, mvPitch, x, y);
    const uint32_t c = texel_u32(curr, currPitch, x, y);
    if (isStatic != 0) atomicMin(keys + (size_t)y * (size_t)W + (size_t)x, kMcStatic);
    if (!matched(prev, prevPitch, c, W, H, x, y, v, matchSad)) return;
    const float s = 1.0f - t;
    const int dx = x + (int)__builtin_floorf((float)v.x * s + 0.5f), dy = y + (int)__builtin_floorf((float)v.y * s + 0.5f);
    if (dx < 0 || dx >= W || dy < 0 || dy >= H) return;
    atomicMin(keys + (size_t)dy * (size_t)W + (size_t)dx, mv_longest_first_key(v.x, v.y));  // result unused: one global_atomic_umin
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_project_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, int W, int H, float t, int matchSad, uint32_t *__restrict__ keys) {
    mc_project<false>(prev, prevPitch, curr, currPitch, mv, mvPitch, nullptr, 0, W, H, t, matchSad, keys);
}

// The two interpolate kernels take their hole walk and the end of a pixel from lfg_mc.hpp (mc_fill_vector,
// mc_store_inside_or_blend), as bidir_sample_kernel does.  They are not one body: what lies between differs in kind (the
// static shortcut, the mask bytes and the fetch rule are the masked kernel's alone) and in place (the unmasked kernel
// computes the clamped position inside the hole branch, the masked one for every pixel).  One template <bool Masked> body
// had to move those, and was not kept.  Each of the two is a body over <bool Plane> under two wrappers:
// the kernel of before, whose machine code the template leaves as it was, and the one that reads the fill plane.
// Plane: a hole takes its vector from the fill plane `fill` (hole_fill.hip), one load, instead of walking K.
template <bool Plane>
__device__ __forceinline__ void mc_interpolate(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ fill, int W,
        int H, float t, int matchSad, uint8_t *__restrict__ out, size_t outPitch) {
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
    // 0: blend as a projected pixel, 1: prev's sample alone (covered), 2: curr's alone (revealed)
    int only = 0;
    if (hole) {
        const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
        const Mv vc = mv_at(mv, mvPitch, cx, cy);
        if (!matched(prev, (size_t)prevPitch, texel_u32(curr, (size_t)currPitch, cx, cy), W, H, cx, cy, vc, matchSad)) only = 2;
        else if (vc.x != u.x || vc.y != u.y) only = 1;
    }
    mc_store_inside_or_blend(sp, tp, sc, tc, only, t, out, outPitch, x, y);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_interpolate_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint32_t *__restrict__ keys, int W, int H, float t, int matchSad,
        uint8_t *__restrict__ out, size_t outPitch) {
    mc_interpolate<false>(prev, prevPitch, curr, currPitch, mv, mvPitch, keys, nullptr, W, H, t, matchSad, out, outPitch);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_interpolate_plane_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ fill, int W,
        int H, float t, int matchSad, uint8_t *__restrict__ out, size_t outPitch) {
    mc_interpolate<true>(prev, prevPitch, curr, currPitch, mv, mvPitch, keys, fill, W, H, t, matchSad, out, outPitch);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_project_masked_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint8_t *__restrict__ mask, size_t maskPitch, int W, int H, float t,
        int matchSad, uint32_t *__restrict__ keys) {
    mc_project<true>(prev, prevPitch, curr, currPitch, mv, mvPitch, mask, maskPitch, W, H, t, matchSad, keys);
}

template <bool Plane>
__device__ __forceinline__ void mc_interpolate_masked(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint8_t *__restrict__ mask, size_t maskPitch,
        const uint32_t *__restrict__ keys, const uint32_t *__restrict__ fill, int W, int H, float t, int matchSad,
        uint8_t *__restrict__ out, size_t outPitch) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const float s = 1.0f - t;
    uint32_t key = keys[(size_t)y * (size_t)W + (size_t)x];
    if (key == kMcStatic) {                                       // the two texels directly: no positions, no gathers
        const V4 p = unorm4(texel_u32(prev, (size_t)prevPitch, x, y)), c = unorm4(texel_u32(curr, (size_t)currPitch, x, y));
        *reinterpret_cast<uint32_t *>(out + (size_t)y * outPitch + (size_t)x * 4u) =
            pack_rgba8_unorm(mixf(p.x, c.x, t), mixf(p.y, c.y, t), mixf(p.z, c.z, t), mixf(p.w, c.w, t));
        return;
    }
    const bool hole = key == kMcHole;
    if (hole) key = Plane ? mc_fill_from_plane(fill, W, x, y) : mc_fill_vector<true>(keys, W, H, x, y);    // the walk also passes over static pixels
    const Mv u = mv_order_decode(key);
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float Px = px + (float)u.x * t, Py = py + (float)u.y * t;
    const float Cx = px - (float)u.x * s, Cy = py - (float)u.y * s;
    const SampleTaps sp = pixel_taps(prev, W, H, prevPitch, Px, Py);
    const SampleTaps sc = pixel_taps(curr, W, H, currPitch, Cx, Cy);
    const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
    const int qx = clampi((int)__builtin_floorf(Px), 0, W - 1), qy = clampi((int)__builtin_floorf(Py), 0, H - 1);
    const SampleTexels tp = sample_load(sp), tc = sample_load(sc);        // eight texels and the two mask bytes in flight
    const uint8_t maskP = mask[(size_t)qy * maskPitch + (size_t)qx], maskC = mask[(size_t)cy * maskPitch + (size_t)cx];
    // 0: blend as a projected pixel, 1: prev's sample alone, 2: curr's alone.  The fetch rule first: content under the overlay
    // in one frame comes from the other.
    int only = (maskP != 0 && maskC == 0) ? 2 : (maskC != 0 && maskP == 0) ? 1 : 0;
    if (only == 0 && hole) {
        const Mv vc = mv_at(mv, mvPitch, cx, cy);
        if (!matched(prev, (size_t)prevPitch, texel_u32(curr, (size_t)currPitch, cx, cy), W, H, cx, cy, vc, matchSad)) only = 2;
        else if (vc.x != u.x || vc.y != u.y) only = 1;
    }
    mc_store_inside_or_blend(sp, tp, sc, tc, only, t, out, outPitch, x, y);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_interpolate_masked_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint8_t *__restrict__ mask, size_t maskPitch,
        const uint32_t *__restrict__ keys, int W, int H, float t, int matchSad, uint8_t *__restrict__ out, size_t outPitch) {
    mc_interpolate_masked<false>(prev, prevPitch, curr, currPitch, mv, mvPitch, mask, maskPitch, keys, nullptr, W, H, t, matchSad, out,
                                 outPitch);
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void mc_interpolate_masked_plane_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint8_t *__restrict__ mask, size_t maskPitch,
        const uint32_t *__restrict__ keys, const uint32_t *__restrict__ fill, int W, int H, float t, int matchSad,
        uint8_t *__restrict__ out, size_t outPitch) {
    mc_interpolate_masked<true>(prev, prevPitch, curr, currPitch, mv, mvPitch, mask, maskPitch, keys, fill, W, H, t, matchSad, out,
                                outPitch);
}

}  // namespace

// Each launcher: clear K, project, interpolate.  With `fill` (lfg_set_hole_reach): clear K, project, the fill plane of `reach`
// into `fill` (W * H words, hole_fill.hip), the interpolate kernel that reads it at holes.
hipError_t launch_interpolate_compensated_masked(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                                 const lfg_mask &mask, const lfg_frame &out, float factor, int matchSad, uint32_t *keys,
                                                 uint32_t *fill, int reach) {
    const int W = (int)curr.width, H = (int)curr.height;
    dim3 grid;
    hipError_t e = mc_clear_keys(s, keys, W, H, grid);
    if (e == hipSuccess)
        e = mc_launch(mc_project_masked_kernel, grid, s, (const uint8_t *)prev.data, (size_t)prev.pitch, (const uint8_t *)curr.data,
                      (size_t)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (const uint8_t *)mask.data,
                      (size_t)mask.pitch, W, H, factor, matchSad, keys);
    if (e == hipSuccess && fill) {
        e = launch_hole_fill_plane(s, keys, (size_t)W, fill, (size_t)W, W, H, reach, true);
        if (e == hipSuccess)
            e = mc_launch(mc_interpolate_masked_plane_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch,
                          (const uint8_t *)curr.data, (int)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch,
                          (const uint8_t *)mask.data, (size_t)mask.pitch, (const uint32_t *)keys, (const uint32_t *)fill, W, H, factor,
                          matchSad, (uint8_t *)out.data, (size_t)out.pitch);
        return e;
    }
    if (e == hipSuccess)
        e = mc_launch(mc_interpolate_masked_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (const uint8_t *)mask.data, (size_t)mask.pitch,
                      (const uint32_t *)keys, W, H, factor, matchSad, (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

// The first half of launch_interpolate_compensated on its own, for a sampling kernel of another file (interpolate_bicubic.hip).
hipError_t launch_compensated_projection(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, float factor,
                                         int matchSad, uint32_t *keys) {
    const int W = (int)curr.width, H = (int)curr.height;
    dim3 grid;
    hipError_t e = mc_clear_keys(s, keys, W, H, grid);
    if (e == hipSuccess)
        e = mc_launch(mc_project_kernel, grid, s, (const uint8_t *)prev.data, (size_t)prev.pitch, (const uint8_t *)curr.data,
                      (size_t)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, W, H, factor, matchSad, keys);
    return e;
}

hipError_t launch_interpolate_compensated(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                          const lfg_frame &out, float factor, int matchSad, uint32_t *keys, uint32_t *fill, int reach) {
    const int W = (int)curr.width, H = (int)curr.height;
    const dim3 grid = mc_grid(W, H);
    hipError_t e = launch_compensated_projection(s, prev, curr, mv, factor, matchSad, keys);
    if (e == hipSuccess && fill) {
        e = launch_hole_fill_plane(s, keys, (size_t)W, fill, (size_t)W, W, H, reach, false);
        if (e == hipSuccess)
            e = mc_launch(mc_interpolate_plane_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                          (int)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (const uint32_t *)keys, (const uint32_t *)fill, W, H,
                          factor, matchSad, (uint8_t *)out.data, (size_t)out.pitch);
        return e;
    }
    if (e == hipSuccess)
        e = mc_launch(mc_interpolate_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (const uint32_t *)keys, W, H, factor, matchSad,
                      (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

}  // namespace lfg
