// What the compensated family shares (interpolate_mc.hip, extrapolate_mc.hip, interpolate_bidir.hip): the key image K's hole
// and static words, the packed-texel read, the vector read, the match gate, the start of every launcher and its launches
// (mc_clear_keys, mc_grid, mc_block, mc_launch), and the two halves that the three sampling kernels which blend both frames
// have in common (mc_interpolate_kernel, mc_interpolate_masked_kernel, bidir_sample_kernel): the hole walk, mc_fill_vector,
// and the end of a pixel, mc_store_inside_or_blend (mc_store_inside_or_blend_values: the same end for interpolate_bicubic.hip's fetch).  Both carry the names of their CPU restatements in
// tests/compensated_model.h.  mc_fill_from_plane is what stands in the walk's place under lfg_set_hole_reach (hole_fill.hip
// makes the plane, tests/fill_model.c restates it), and kFillBand is that file's band height.  The vector word, the longest-first key that K holds (mv_longest_first_key), its decode
// (mv_order_decode) and the hole walks' way back to the order key (mv_key_flip_length) are lfg_vector_word.hpp's; the taps
// are lfg_interp.hpp's.  The sub-pixel route's reads, gate and walk (interpolate_subpel.hip) are new functions at the end.
#pragma once

#include "lfg_device.hpp"
#include "lfg_internal.hpp"
#include "lfg_interp.hpp"
#include "lfg_vector_word.hpp"

namespace lfg {

constexpr uint32_t kMcHole = 0xFFFFFFFFu;      // K where nothing was projected: what the clear leaves, above every key
// Key 0 marks a static location (the masked pair only): no vector's key is 0 (65535 - |v|^2 >= 32767), and it is the smallest
// word, so it outlasts whatever is projected onto it.
constexpr uint32_t kMcStatic = 0u;
constexpr int kMcWalk = 16;                    // every hole walk's reach, per axis direction
constexpr int kMcBlockX = 64, kMcBlockY = 4;   // a wave is 64 pixels of one row

__device__ __forceinline__ uint32_t texel_u32(const uint8_t *__restrict__ img, size_t pitch, int x, int y) {
    return *reinterpret_cast<const uint32_t *>(img + (size_t)y * pitch + (size_t)x * 4u);
}

__device__ __forceinline__ Mv mv_at(const uint8_t *__restrict__ mv, size_t pitch, int x, int y) {
    return mv_unpack(*reinterpret_cast<const uint16_t *>(mv + (size_t)y * pitch + (size_t)x * 2u));
}

// The match gate: sum over the channels of |curr(q) - prev(q + v)| <= matchSad, prev outside the image read as 0.
// (pair_stats.hip counts the same comparison, on texels it has loaded a trip ahead.)
__device__ __forceinline__ bool matched(const uint8_t *__restrict__ prev, size_t prevPitch, uint32_t currTexel,
                                        int W, int H, int qx, int qy, Mv v, int matchSad) {
    const int sx = qx + v.x, sy = qy + v.y;
    const uint32_t p = (sx >= 0 && sx < W && sy >= 0 && sy < H) ? texel_u32(prev, prevPitch, sx, sy) : 0u;
    return __builtin_amdgcn_sad_u8(currTexel, p, 0u) <= (uint32_t)matchSad;
}

// The fill vector of hole (x, y), as its order key: of the first non-hole word in each axis direction within kMcWalk, the
// smallest (|v|^2, vy, vx); (0, 0) when every direction runs out.  Only the low 16 bits of the result are decoded.
// PassStatic (the masked kernel): the walk also passes over static pixels, an overlay is not the surface behind it.
// (ex_sample_kernel's batched walk is another algorithm: it keeps the step count for the donor.)
template <bool PassStatic>
__device__ __forceinline__ uint32_t mc_fill_vector(const uint32_t *__restrict__ keys, int W, int H, int x, int y) {
    uint32_t best = kMcHole;
    const int stepX[4] = {1, -1, 0, 0}, stepY[4] = {0, 0, 1, -1};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        for (int k = 1; k <= kMcWalk; ++k) {
            const int nx = x + stepX[d] * k, ny = y + stepY[d] * k;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
            const uint32_t n = keys[(size_t)ny * (size_t)W + (size_t)nx];
            if (n == kMcHole || (PassStatic && n == kMcStatic)) continue;
            const uint32_t order = mv_key_flip_length(n);
            best = order < best ? order : best;
            break;
        }
    }
    return best == kMcHole ? mv_order_key(0, 0) : best;
}

// The same from the fill plane (hole_fill.hip; lfg_set_hole_reach): the plane holds the order key already, and the hole word
// where no direction has a donor within the reach.  One load in the walk's place.
__device__ __forceinline__ uint32_t mc_fill_from_plane(const uint32_t *__restrict__ fill, int W, int x, int y) {
    const uint32_t best = fill[(size_t)y * (size_t)W + (size_t)x];
    return best == kMcHole ? mv_order_key(0, 0) : best;
}
constexpr int kFillBand = 64;                  // rows per workgroup of the plane's column pass

// The end of an interpolated pixel.  `only` is what the caller's rules decided -- 0: nothing, 1: prev's sample alone, 2:
// curr's alone -- and 0 falls to the inside rule: the sample whose position alone is inside the image, else the blend.
__device__ __forceinline__ void mc_store_inside_or_blend(const SampleTaps &sp, const SampleTexels &tp, const SampleTaps &sc,
                                                         const SampleTexels &tc, int only, float t, uint8_t *__restrict__ out,
                                                         size_t outPitch, int x, int y) {
    if (only == 0) only = sp.inside && !sc.inside ? 1 : (sc.inside && !sp.inside ? 2 : 0);
    const V4 P = blend_taps(sp, tp), C = blend_taps(sc, tc);
    const V4 r = only == 1 ? P : only == 2 ? C : V4{mixf(P.x, C.x, t), mixf(P.y, C.y, t), mixf(P.z, C.z, t), mixf(P.w, C.w, t)};
    *reinterpret_cast<uint32_t *>(out + (size_t)y * outPitch + (size_t)x * 4u) = pack_rgba8_unorm(r.x, r.y, r.z, r.w);
}

// The same end from two sample values and their inside flags, for a fetch that is not blend_taps (interpolate_bicubic.hip): the
// decision, mixf and the store are mc_store_inside_or_blend's.
__device__ __forceinline__ void mc_store_inside_or_blend_values(const V4 &P, bool pInside, const V4 &C, bool cInside, int only, float t,
                                                                uint8_t *__restrict__ out, size_t outPitch, int x, int y) {
    if (only == 0) only = pInside && !cInside ? 1 : (cInside && !pInside ? 2 : 0);
    const V4 r = only == 1 ? P : only == 2 ? C : V4{mixf(P.x, C.x, t), mixf(P.y, C.y, t), mixf(P.z, C.z, t), mixf(P.w, C.w, t)};
    *reinterpret_cast<uint32_t *>(out + (size_t)y * outPitch + (size_t)x * 4u) = pack_rgba8_unorm(r.x, r.y, r.z, r.w);
}

// ---- the sub-pixel route (interpolate_subpel.hip; tests/subpel_model.c restates these): quarter-pixel vectors, a key image
// of 64-bit words.
constexpr unsigned long long kMcqHole = ~0ull;   // what the clear leaves, above every key (lfg_vector_word.hpp)

__device__ __forceinline__ Mv mvq_at(const uint8_t *__restrict__ mvq, size_t pitch, int x, int y) {
    return mvq_unpack(*reinterpret_cast<const uint32_t *>(mvq + (size_t)y * pitch + (size_t)x * 4u));
}

// prevq(r, w), lfg_motion_subpel's fractional sample, as a packed texel: the four texels at r + (w >> 2) and one step right
// and down, outside the image read as 0, weighted by the quarters (w & 3); per channel (sum + 8) >> 4.  Channels 0 and 2 /
// 1 and 3 travel in 16-bit halves: a sum stays below 255 * 16 + 8.
__device__ __forceinline__ uint32_t prevq_texel(const uint8_t *__restrict__ prev, size_t prevPitch, int W, int H, int rx, int ry, Mv w) {
    const int ix = rx + (w.x >> 2), iy = ry + (w.y >> 2);
    const uint32_t fx = (uint32_t)(w.x & 3), fy = (uint32_t)(w.y & 3);
    const uint32_t t00 = texel_or_zero(prev, prevPitch, ix, iy, W, H), t10 = texel_or_zero(prev, prevPitch, ix + 1, iy, W, H);
    const uint32_t t01 = texel_or_zero(prev, prevPitch, ix, iy + 1, W, H), t11 = texel_or_zero(prev, prevPitch, ix + 1, iy + 1, W, H);
    const uint32_t w00 = (4u - fx) * (4u - fy), w10 = fx * (4u - fy), w01 = (4u - fx) * fy, w11 = fx * fy;
    const uint32_t even = (t00 & 0x00FF00FFu) * w00 + (t10 & 0x00FF00FFu) * w10 + (t01 & 0x00FF00FFu) * w01 + (t11 & 0x00FF00FFu) * w11 + 0x00080008u;
    const uint32_t odd = ((t00 >> 8) & 0x00FF00FFu) * w00 + ((t10 >> 8) & 0x00FF00FFu) * w10 + ((t01 >> 8) & 0x00FF00FFu) * w01 +
                         ((t11 >> 8) & 0x00FF00FFu) * w11 + 0x00080008u;
    return ((even >> 4) & 0x00FF00FFu) | (((odd >> 4) & 0x00FF00FFu) << 8);
}

// The fractional match gate: sum over the channels of |curr(q) - prevq(q, w)| <= matchSad.
__device__ __forceinline__ bool matched_q(const uint8_t *__restrict__ prev, size_t prevPitch, uint32_t currTexel, int W, int H, int qx,
                                          int qy, Mv w, int matchSad) {
    return __builtin_amdgcn_sad_u8(currTexel, prevq_texel(prev, prevPitch, W, H, qx, qy, w), 0u) <= (uint32_t)matchSad;
}

// mc_fill_vector over the 64-bit key image, as the order key: the smallest (|w|^2, wy, wx) of the first non-hole word in each
// axis direction within kMcWalk; (0, 0) when every direction runs out.
__device__ __forceinline__ unsigned long long mcq_fill_vector(const unsigned long long *__restrict__ keys, int W, int H, int x, int y) {
    unsigned long long best = kMcqHole;
    const int stepX[4] = {1, -1, 0, 0}, stepY[4] = {0, 0, 1, -1};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        for (int k = 1; k <= kMcWalk; ++k) {
            const int nx = x + stepX[d] * k, ny = y + stepY[d] * k;
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) break;
            const unsigned long long n = keys[(size_t)ny * (size_t)W + (size_t)nx];
            if (n == kMcqHole) continue;
            const unsigned long long order = mvq_key_flip_length(n);
            best = order < best ? order : best;
            break;
        }
    }
    return best == kMcqHole ? mvq_order_key(0, 0) : best;
}

// Every launcher's start: K (W * H words) set to the hole word in stream order, and the grid of every launch, one thread
// per pixel in blocks of kMcBlockX x kMcBlockY.  mc_launch is one launch on that grid and its error.
inline dim3 mc_block() { return dim3(kMcBlockX, kMcBlockY); }
inline dim3 mc_grid(int W, int H) {
    return dim3((unsigned)((W + kMcBlockX - 1) / kMcBlockX), (unsigned)((H + kMcBlockY - 1) / kMcBlockY));
}
inline hipError_t mc_clear_keys(hipStream_t s, uint32_t *keys, int W, int H, dim3 &grid) {
    grid = mc_grid(W, H);
    return hipMemsetAsync(keys, 0xFF, (size_t)W * (size_t)H * 4u, s);
}
template <typename... Params, typename... Args>
inline hipError_t mc_launch(void (*kernel)(Params...), dim3 grid, hipStream_t s, Args... args) {
    hipLaunchKernelGGL(kernel, grid, mc_block(), 0, s, args...);
    return hipGetLastError();
}

}  // namespace lfg
