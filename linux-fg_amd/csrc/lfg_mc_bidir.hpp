// What the bidirectional kernels share (interpolate_bidir.hip): the forward-backward check of a vector and the two
// `confirmed` predicates built on it and on lfg_mc.hpp's match gate.  The contract (include/linuxfg_hip.h restates it):
//
//   fwd   LFG_FORMAT_MV_S8X2 on curr's grid, as lfg_motion(prev, curr) writes it: prev(q + f) ~ curr(q);
//   bwd   on prev's grid, as lfg_motion(curr, prev) writes it: curr(p + b) ~ prev(p).
//   Any byte values; components are integers in [-128, 127]; everything below is integer arithmetic.
//
//   consistent(a, other, q)   r = q + a lies inside the image and |a.x + other(r).x| + |a.y + other(r).y| <= tolerance
//                             (the L1 distance between a and the negated vector measured the other way at a's far end);
//   confirmed_f(q), f = fwd(q)   the match gate sum_c |curr(q)_c - prev(q + f)_c| <= match_sad (prev outside read as 0)
//                                and consistent(f, bwd, q);
//   confirmed_b(p), b = bwd(p)   the gate sum_c |prev(p)_c - curr(p + b)_c| <= match_sad (curr outside read as 0),
//                                consistent(b, fwd, p), and neither component of b is -128: its negation, the vector
//                                the content of p carries in fwd's convention, does not fit the vector word.
//
// A vector that only the gate lets through -- any vector on flat or repetitive content -- is not confirmed unless the
// field measured the other way agrees with it.  tests/bidir_model.c restates all of this on the CPU.
#pragma once

#include "lfg_mc.hpp"

namespace lfg {

__device__ __forceinline__ int bidir_absi(int v) { return v < 0 ? -v : v; }

// The vector half: `a` at (x, y) against `other`, the field measured the other way.  One 2-byte gather.
__device__ __forceinline__ bool bidir_consistent(const uint8_t *__restrict__ other, size_t otherPitch, int W, int H, int x, int y,
                                                 Mv a, int tolerance) {
    const int rx = x + a.x, ry = y + a.y;
    if (rx < 0 || rx >= W || ry < 0 || ry >= H) return false;
    const Mv o = mv_at(other, otherPitch, rx, ry);
    return bidir_absi(a.x + o.x) + bidir_absi(a.y + o.y) <= tolerance;
}

// confirmed_f with (far, own's texel, fwd(q), bwd); confirmed_b with (curr as `far`, prev's texel, bwd(p), fwd) and Backward.
template <bool Backward>
__device__ __forceinline__ bool bidir_confirmed(const uint8_t *__restrict__ far, size_t farPitch, uint32_t ownTexel,
                                                const uint8_t *__restrict__ other, size_t otherPitch, int W, int H, int x, int y,
                                                Mv a, int matchSad, int tolerance) {
    if (Backward && (a.x == -128 || a.y == -128)) return false;
    return matched(far, farPitch, ownTexel, W, H, x, y, a, matchSad) && bidir_consistent(other, otherPitch, W, H, x, y, a, tolerance);
}

}  // namespace lfg
