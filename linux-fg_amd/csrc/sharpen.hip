// sharpen.hip -- contrast-limited sharpening of an RGBA8 frame (lfg_sharpen, include/linuxfg_hip.h).  No reference counterpart;
// opt-in, outside the three stages, at the presentation end.  tests/sharpen_model.py restates the definition on the CPU.
//
// sharpen_kernel  per pixel and channel the 5-point Laplacian L = 4 C - N - S - W - E, scaled by strength / 64 (rounded, floor
//                 shift), added to C and limited to the range of the five inputs.  4 bytes read, 4 written per pixel.
//
// A memory-bound stencil.  The shape:
//   * An item is four pixels of one row through one 16-byte load and one 16-byte store (kWide), chosen by the host when base
//     and pitch of BOTH frames are multiples of 16; otherwise an item is one pixel through dword accesses.  An item is never
//     partial: of a width that is no multiple of 4 the wide launch takes the columns up to the last multiple, and a second
//     launch of the dword kernel the 1 .. 3 columns that remain (launch_sharpen; lfg_record_plan.hpp: wide_columns).
//   * A lane takes a STRIP of kSharpenRows rows of its item, top to bottom: the kSharpenRows + 2 rows it needs (one halo row
//     above and one below, clamped to the frame) are each loaded once, all of them before the first use of any, so a lane has
//     its whole strip in flight at once; rows y - 1, y, y + 1 of an output row are then registers.  Per strip 10 rows are
//     fetched for 8 written: the two halo rows are the neighbouring strips' own rows and come from the caches.
//   * The texels left and right of an item (x - 1 and x + 4, clamped to the frame) are dword loads of their own; they hit the
//     lines the neighbouring lanes fetch.  No LDS and no cross-lane operation: tests/cpp/sharpen_on_host.cpp compiles this file
//     for the CPU and runs a launch as loops.
//   * A wave is 64 consecutive items of one strip -- 1 KiB of each row where the items are wide -- and a workgroup four waves
//     on four strips one below the other, whose shared halo rows meet in the CU's L1.  The grid is derived from the size:
//     x counts groups of four strips, y groups of 64 items (past 65,535 of them a workgroup walks on by gridDim.y).
//   * Byte offsets are size_t throughout: a frame of 2 GiB and more is addressed like any other.
// No data-dependent branch: the cost does not depend on the content, nor on the strength (0 copies through the same code).
// No float anywhere.  |strength * L + 32| <= 65,312: 32-bit integers.
//
// Traffic per pixel: 4 + 4 = 8 bytes, 66.4 MB at 4K.
#ifndef LFG_SHARPEN_ON_HOST                                  // tests/cpp/sharpen_on_host.cpp compiles the kernels for the CPU, with its
#include "lfg_internal.hpp"                                 // own stand-ins for what these two headers and the HIP runtime give them
#include "lfg_device.hpp"
#endif
#include "lfg_record_plan.hpp"                              // (standard library only: the host build takes it as well)

namespace lfg {
namespace {

constexpr int kSharpenRows = 8;                             // R: output rows of a strip
constexpr int kSharpenWaveItems = 64;                       // items of one strip per wave
constexpr int kSharpenGroupStrips = 4;                      // strips (waves) per workgroup, one below the other
constexpr uint32_t kSharpenMaxGridY = 65535u;

__host__ __device__ __forceinline__ int sharpen_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int sharpen_max(int a, int b) { return a > b ? a : b; }

// strength * L: |L| <= 1020 and strength <= 64 fit the full-rate 24-bit multiply; the compiler, which does not know the
// range of a kernel argument, would take the quarter-rate 64-bit multiply-add.
__host__ __device__ __forceinline__ int sharpen_scaled(int strength, int L) {
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(strength, L);
#else
    return strength * L;
#endif
}

// The definition, for one channel: the centre C and its four neighbours, all bytes; 0 <= strength <= 64.
__host__ __device__ __forceinline__ int sharpen_channel(int C, int N, int S, int W, int E, int strength) {
    const int L = 4 * C - N - S - W - E;
    const int lo = sharpen_min(sharpen_min(sharpen_min(C, N), sharpen_min(S, W)), E);
    const int hi = sharpen_max(sharpen_max(sharpen_max(C, N), sharpen_max(S, W)), E);
    const int v = C + ((sharpen_scaled(strength, L) + 32) >> 6);           // (arithmetic shift: floor)
    return sharpen_min(sharpen_max(v, lo), hi);
}

// All four channels of one texel.  The result of sharpen_channel is limited to [lo, hi], not to a constant byte range, so
// this is not the shift-clamp-pack pattern that yuv_convert.hip keeps apart; the build's check of the machine code
// (check_store_hazard.py) would refuse it if it were.
__host__ __device__ __forceinline__ uint32_t sharpen_texel(uint32_t c, uint32_t n, uint32_t s, uint32_t w, uint32_t e, int strength) {
    uint32_t px = 0u;
#pragma unroll
    for (int k = 0; k < 32; k += 8)
        px |= (uint32_t)sharpen_channel((int)((c >> k) & 255u), (int)((n >> k) & 255u), (int)((s >> k) & 255u), (int)((w >> k) & 255u),
                                        (int)((e >> k) & 255u), strength) << k;
    return px;
}

#ifndef LFG_SHARPEN_ON_HOST
// threadIdx.y is the same for the 64 lanes of a wave (the workgroup is 64 wide), which the compiler cannot know: said
// here, the strip's row addresses are scalar arithmetic.
__device__ __forceinline__ uint32_t wave_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
#endif

template <bool kWide>
__global__ __launch_bounds__(kSharpenWaveItems * kSharpenGroupStrips) void sharpen_kernel(
        const uint8_t *__restrict__ in, size_t inPitch, uint8_t *__restrict__ out, size_t outPitch, uint32_t W, uint32_t H,
        uint32_t xFirst, uint32_t itemsX, int strength) {
    constexpr uint32_t kPixels = kWide ? 4u : 1u;
    constexpr int R = kSharpenRows;
    // this wave's strip: rows y0 .. y0 + R - 1, those below H
    const size_t y0 = ((size_t)blockIdx.x * kSharpenGroupStrips + wave_uniform(threadIdx.y)) * (size_t)R;
    if (y0 >= (size_t)H) return;
    const size_t last = (size_t)H - 1u;
    const size_t groupsX = ((size_t)itemsX + kSharpenWaveItems - 1u) / kSharpenWaveItems;
    for (size_t gx = blockIdx.y; gx < groupsX; gx += gridDim.y) {
        const size_t g = gx * kSharpenWaveItems + threadIdx.x;
        if (g >= (size_t)itemsX) continue;
        // the item's first pixel, and the texels left and right of the item, clamped to the frame
        const uint32_t x = xFirst + (uint32_t)g * kPixels;
        const size_t centre = (size_t)x * 4u, left = (size_t)(x > 0u ? x - 1u : 0u) * 4u;
        const size_t right = (size_t)(x + kPixels < W ? x + kPixels : W - 1u) * 4u;

        // every load of the strip, before the first use of any: row k is y0 + k - 1, clamped to the frame
        uint32_t c[R + 2][kPixels], l[R], r[R];
#pragma unroll
        for (int k = 0; k < R + 2; ++k) {
            const size_t y = k == 0 ? (y0 > 0u ? y0 - 1u : 0u) : (y0 + (size_t)(k - 1) < last ? y0 + (size_t)(k - 1) : last);
            const uint8_t *__restrict__ row = in + y * inPitch;
            if constexpr (kWide) {
                const uint4 v = *reinterpret_cast<const uint4 *>(row + centre);
                c[k][0] = v.x; c[k][1] = v.y; c[k][2] = v.z; c[k][3] = v.w;
            } else {
                c[k][0] = *reinterpret_cast<const uint32_t *>(row + centre);
            }
            if (k >= 1 && k <= R) {
                l[k - 1] = *reinterpret_cast<const uint32_t *>(row + left);
                r[k - 1] = *reinterpret_cast<const uint32_t *>(row + right);
            }
        }

        uint8_t *__restrict__ o = out + y0 * outPitch + centre;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            if (y0 + (size_t)j <= last) {                    // (wave-uniform)
                uint32_t px[kPixels];
#pragma unroll
                for (uint32_t i = 0; i < kPixels; ++i) {
                    const uint32_t w = i > 0u ? c[j + 1][i > 0u ? i - 1u : 0u] : l[j];
                    const uint32_t e = i + 1u < kPixels ? c[j + 1][i + 1u < kPixels ? i + 1u : 0u] : r[j];
                    px[i] = sharpen_texel(c[j + 1][i], c[j][i], c[j + 2][i], w, e, strength);
                }
                if constexpr (kWide) store_16_guarded(o, uint4{px[0], px[1], px[2], px[3]});
                else *reinterpret_cast<uint32_t *>(o) = px[0];
            }
            o += outPitch;
        }
    }
}

// What lfg_sharpen launches, as plain C++ (tests/cpp/sharpen_on_host.cpp runs the same parts as loops): the dword kernel over
// everything, or -- base and pitch of both frames multiples of 16 -- the 16-byte kernel over the columns up to the last
// multiple of 4 and the dword kernel over the 1 .. 3 that remain.  The parts write disjoint bytes and read only `in`, whose
// neighbours they clamp to the whole frame, not to their own columns.
struct SharpenPart { bool wide; uint32_t xFirst, itemsX, gridX, gridY; };

inline SharpenPart sharpen_part(bool wide, uint32_t xFirst, uint32_t cols, uint32_t H) {
    const uint32_t itemsX = wide ? cols / 4u : cols;
    const unsigned long long groupsX = ((unsigned long long)itemsX + kSharpenWaveItems - 1u) / kSharpenWaveItems;
    const unsigned long long rowsPerGroup = (unsigned long long)kSharpenRows * kSharpenGroupStrips;
    const unsigned long long stripGroups = ((unsigned long long)H + rowsPerGroup - 1u) / rowsPerGroup;              // < 2^27
    return SharpenPart{wide, xFirst, itemsX, (uint32_t)stripGroups, (uint32_t)(groupsX < kSharpenMaxGridY ? groupsX : kSharpenMaxGridY)};
}

inline int sharpen_parts(const void *in, size_t inPitch, const void *out, size_t outPitch, uint32_t W, uint32_t H, SharpenPart (&parts)[2]) {
    const uint32_t wideW = wide_columns(multiples_of_16(in, out, inPitch, outPitch), W);
    int n = 0;
    if (wideW != 0u) parts[n++] = sharpen_part(true, 0u, wideW, H);
    if (wideW != W) parts[n++] = sharpen_part(false, wideW, W - wideW, H);
    return n;
}

}  // namespace

#ifndef LFG_SHARPEN_ON_HOST
hipError_t launch_sharpen(hipStream_t s, const lfg_frame &in, const lfg_frame &out, int strength) {
    SharpenPart parts[2];
    const int n = sharpen_parts(in.data, in.pitch, out.data, out.pitch, in.width, in.height, parts);
    for (int i = 0; i < n; ++i) {
        const SharpenPart &p = parts[i];
        const auto kernel = p.wide ? sharpen_kernel<true> : sharpen_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(p.gridX, p.gridY), dim3(kSharpenWaveItems, kSharpenGroupStrips), 0, s, (const uint8_t *)in.data,
                           (size_t)in.pitch, (uint8_t *)out.data, (size_t)out.pitch, in.width, in.height, p.xFirst, p.itemsX, strength);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
#endif

}  // namespace lfg
