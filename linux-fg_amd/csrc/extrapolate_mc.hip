// extrapolate_mc.hip -- motion-compensated extrapolation (lfg_extrapolate_compensated, include/linuxfg_hip.h): curr's content is
// projected past time 1 along the vectors just measured, and curr alone is fetched along the projected vectors.  No reference
// counterpart; opt-in, next to interpolate_mc.hip, with which it shares the hole word, the walk's reach, the reads, the match
// gate and the launcher's steps (lfg_mc.hpp) and the key with its decode (lfg_vector_word.hpp); the batched hole walk is its own.
// tests/extrapolate_model.c restates every step below on the CPU.
//
// Two launches per factor, after the key image K (W * H words, the lane's scratch, interpolate_mc.hip's) has been set to 0xFF
// bytes in stream order:
//   ex_project_kernel   one thread per source pixel q: the match gate, then one atomicMin of the vector's key into K(q - v a);
//   ex_sample_kernel    one thread per output pixel: K, the hole walk and the donor rule where K is a hole, one bilinear fetch.
// The second launch starts once every projection is visible, and it never writes K.
//
// Traffic per pixel and factor: 4 (clear) + 2 (mv) + 4 (curr) + 4 (gathered prev) + 4 (atomic) in the projection, 4 (K) + 4
// (one fetch, mostly cached neighbours) + 4 (out) in the sampling: 30 bytes, 249 MB at 4K.
#include "lfg_mc.hpp"

namespace lfg {

namespace {

constexpr int kExBatch = 4;                    // words of each direction loaded ahead of their comparison

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void ex_project_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, int W, int H, float a, int matchSad, uint32_t *__restrict__ keys) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const Mv v = mv_at(mv, mvPitch, x, y);
    if (!matched(prev, prevPitch, texel_u32(curr, currPitch, x, y), W, H, x, y, v, matchSad)) return;
    // content at q came from q + v: it moves by -v per interval
    const int dx = x + (int)__builtin_floorf(0.5f - (float)v.x * a), dy = y + (int)__builtin_floorf(0.5f - (float)v.y * a);
    if (dx < 0 || dx >= W || dy < 0 || dy >= H) return;
    atomicMin(keys + (size_t)dy * (size_t)W + (size_t)dx, mv_longest_first_key(v.x, v.y));  // result unused: one global_atomic_umin
}

__global__ __launch_bounds__(kMcBlockX * kMcBlockY) void ex_sample_kernel(
        const uint8_t *__restrict__ prev, int prevPitch, const uint8_t *__restrict__ curr, int currPitch,
        const uint8_t *__restrict__ mv, size_t mvPitch, const uint32_t *__restrict__ keys, int W, int H, float a, int matchSad,
        uint8_t *__restrict__ out, size_t outPitch) {
    const int x = (int)(blockIdx.x * kMcBlockX + threadIdx.x), y = (int)(blockIdx.y * kMcBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    uint32_t key = keys[(size_t)y * (size_t)W + (size_t)x];
    const bool hole = key == kMcHole;
    bool donor = false;
    int nx = x, ny = y;
    if (hole) {
        // Each direction's first non-hole word within kMcWalk.  The words of all four directions are loaded kExBatch steps
        // ahead of their comparison: a round is 16 independent loads, and a hole next to projected pixels is done after one.
        // A step past the image edge reads as a hole (its address is clamped into the image): every later step of that
        // direction is past the edge too, so the direction keeps nothing, as when the walk stops there.
        const int stepX[4] = {1, -1, 0, 0}, stepY[4] = {0, 0, 1, -1};
        uint32_t first[4] = {kMcHole, kMcHole, kMcHole, kMcHole};
        int firstK[4] = {0, 0, 0, 0};
        for (int base = 1; base <= kMcWalk; base += kExBatch) {
            uint32_t n[4][kExBatch];
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int j = 0; j < kExBatch; ++j) {
                    const int qx = x + stepX[d] * (base + j), qy = y + stepY[d] * (base + j);
                    n[d][j] = keys[(size_t)clampi(qy, 0, H - 1) * (size_t)W + (size_t)clampi(qx, 0, W - 1)];
                }
            bool all = true;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
#pragma unroll
                for (int j = 0; j < kExBatch; ++j) {
                    const int qx = x + stepX[d] * (base + j), qy = y + stepY[d] * (base + j);
                    const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                    if (first[d] == kMcHole && in && n[d][j] != kMcHole) { first[d] = n[d][j]; firstK[d] = base + j; }
                }
                all = all && first[d] != kMcHole;
            }
            if (all) break;
        }
        // The fill vector: the smallest (|v|^2, vy, vx) of the kept words; on an equal triple the earlier direction stays.
        // (0, 0) and no donor when every direction ran out.
        uint32_t best = kMcHole;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (first[d] == kMcHole) continue;
            const uint32_t order = mv_key_flip_length(first[d]);
            if (order < best) { best = order; nx = x + stepX[d] * firstK[d]; ny = y + stepY[d] * firstK[d]; }
        }
        donor = best != kMcHole;
        key = donor ? best : mv_order_key(0, 0);               // only the low 16 bits are decoded
    }
    const Mv u = mv_order_decode(key);
    const float Cx = px + (float)u.x * a, Cy = py + (float)u.y * a;
    SampleTaps sc = pixel_taps(curr, W, H, currPitch, Cx, Cy);
    SampleTexels tc = sample_load(sc);
    if (donor) {
        // The gate at c and the fetch from the donor's own position, all in flight together; which fetch is used is decided
        // once the gate is known.
        const int cx = clampi((int)__builtin_floorf(Cx), 0, W - 1), cy = clampi((int)__builtin_floorf(Cy), 0, H - 1);
        const float Nx = ((float)nx + 0.5f) + (float)u.x * a, Ny = ((float)ny + 0.5f) + (float)u.y * a;
        const SampleTaps sn = pixel_taps(curr, W, H, currPitch, Nx, Ny);
        const Mv vc = mv_at(mv, mvPitch, cx, cy);
        const uint32_t cTexel = texel_u32(curr, (size_t)currPitch, cx, cy);
        const SampleTexels tn = sample_load(sn);
        // curr shows the foreground at c, and the surface behind it is in neither frame: the background's edge is stretched
        if (matched(prev, (size_t)prevPitch, cTexel, W, H, cx, cy, vc, matchSad) && (vc.x != u.x || vc.y != u.y)) {
            sc = sn;
            tc = tn;
        }
    }
    const V4 r = blend_taps(sc, tc);
    *reinterpret_cast<uint32_t *>(out + (size_t)y * outPitch + (size_t)x * 4u) = pack_rgba8_unorm(r.x, r.y, r.z, r.w);
}

}  // namespace

hipError_t launch_extrapolate_compensated(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                          const lfg_frame &out, float ahead, int matchSad, uint32_t *keys) {
    const int W = (int)curr.width, H = (int)curr.height;
    dim3 grid;
    hipError_t e = mc_clear_keys(s, keys, W, H, grid);
    if (e == hipSuccess)
        e = mc_launch(ex_project_kernel, grid, s, (const uint8_t *)prev.data, (size_t)prev.pitch, (const uint8_t *)curr.data,
                      (size_t)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, W, H, ahead, matchSad, keys);
    if (e == hipSuccess)
        e = mc_launch(ex_sample_kernel, grid, s, (const uint8_t *)prev.data, (int)prev.pitch, (const uint8_t *)curr.data,
                      (int)curr.pitch, (const uint8_t *)mv.data, (size_t)mv.pitch, (const uint32_t *)keys, W, H, ahead, matchSad,
                      (uint8_t *)out.data, (size_t)out.pitch);
    return e;
}

}  // namespace lfg
