// deband.hip -- debanding with dithered output of an RGBA8 frame (lfg_deband, include/linuxfg_hip.h).  No reference
// counterpart; opt-in, outside the three stages, at the presentation end behind lfg_sharpen.  tests/deband_model.py restates
// the definition on the CPU, and lfg_deband.hpp holds the per-pixel rule that the kernel shares with lfg_deband_draw and with
// the CPU run of this file (tests/cpp/deband_on_host.cpp compiles it as it is).
//
// deband_kernel  per pixel I iterations, each the sum of four taps of `in` at a random offset and its three quarter turns
//                (clamped to the frame), accepted where it lies within the threshold of the running value; then noise and the
//                rounding to 8 bits.  4 bytes read at the pixel, 4 written, 4 I gathered dwords.
//
// A gather.  The shape:
//   * An item is four pixels of one row through one 16-byte load and one 16-byte store (kWide), chosen by the host when base
//     and pitch of BOTH frames are multiples of 16; otherwise an item is one pixel through dword accesses.  An item is never
//     partial: of a width that is no multiple of 4 the wide launch takes the columns up to the last multiple, and a second
//     launch of the dword kernel the 1 .. 3 columns that remain (launch_deband; lfg_record_plan.hpp: wide_columns).
//   * A wave is 64 consecutive items of one row -- 1 KiB of it where the items are wide -- and a workgroup four waves on four
//     rows one below the other, whose taps meet in the CU's L1: at radius R the taps of iteration i lie within R i rows and
//     columns of the pixel.  The grid is derived from the size: x counts groups of four rows, y groups of 64 items (past
//     65,535 of them a workgroup walks on by gridDim.y).
//   * Every tap of an item -- 4 I per pixel, from clamped positions, so no load is conditional -- is issued before the first is
//     used.  The kernel is instantiated by I: the loads are a fixed, unrolled set.
//   * The draw is lfg_deband.hpp's: h(seed) comes from the host, the row's key is the same for a wave (scalar arithmetic),
//     and a pixel takes one hash for r0 and one per iteration and for the noise.  The offset and noise products fit the 24-bit
//     multiply; the hash's two multiplies are full 32-bit ones.
//   * Byte offsets are size_t throughout: a frame of 2 GiB and more is addressed like any other.  A tap's offset is one
//     32 x 32 -> 64 bit multiply-add (the pitch is a 32-bit field of lfg_frame).
// No LDS and no cross-lane operation but the row's readfirstlane; no data-dependent branch or exit: the cost does not depend
// on the content, nor on threshold and grain (threshold 0 with grain 0 copies through the same code).  No float anywhere.
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_deband.hpp"
#include "lfg_record_plan.hpp"

namespace lfg {
namespace {

constexpr int kDebandWaveItems = 64;                        // items of one row per wave
constexpr int kDebandGroupRows = 4;                         // rows (waves) per workgroup, one below the other
constexpr uint32_t kDebandMaxGridY = 65535u;

// threadIdx.y is the same for the 64 lanes of a wave (the workgroup is 64 wide), which the compiler cannot know: said here,
// the row's key and the row's address are scalar arithmetic.
__device__ __forceinline__ uint32_t deband_wave_uniform(uint32_t v) {
#ifdef LFG_ON_HOST
    return v;
#else
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#endif
}

template <int I, bool kWide>
__global__ __launch_bounds__(kDebandWaveItems * kDebandGroupRows) void deband_kernel(
        const uint8_t *__restrict__ in, uint32_t inPitch, uint8_t *__restrict__ out, uint32_t outPitch, uint32_t W, uint32_t H,
        uint32_t xFirst, uint32_t itemsX, int threshold, int radius, int grain, uint32_t seedKey) {
    constexpr uint32_t kPixels = kWide ? 4u : 1u;
    constexpr int kTaps = kDebandTaps * I;
    // this wave's row
    const size_t row = (size_t)blockIdx.x * kDebandGroupRows + deband_wave_uniform(threadIdx.y);
    if (row >= (size_t)H) return;
    const uint32_t y = (uint32_t)row;
    const uint32_t rowKey = deband_row_key(seedKey, y);
    const uint8_t *__restrict__ inRow = in + row * inPitch;
    uint8_t *__restrict__ outRow = out + row * outPitch;
    const size_t groupsX = ((size_t)itemsX + kDebandWaveItems - 1u) / kDebandWaveItems;
    for (size_t gx = blockIdx.y; gx < groupsX; gx += gridDim.y) {
        const size_t g = gx * kDebandWaveItems + threadIdx.x;
        if (g >= (size_t)itemsX) continue;
        const uint32_t x = xFirst + (uint32_t)g * kPixels;

        // every load of the item, before the first use of any
        uint32_t c[kPixels], noise[kPixels], taps[kPixels][kTaps];
        if constexpr (kWide) {
            const uint4 v = *reinterpret_cast<const uint4 *>(inRow + (size_t)x * 4u);
            c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
        } else {
            c[0] = *reinterpret_cast<const uint32_t *>(inRow + (size_t)x * 4u);
        }
#pragma unroll
        for (uint32_t p = 0; p < kPixels; ++p) {
            const uint32_t r0 = deband_r0(rowKey, x + p);
            noise[p] = deband_r(r0, kDebandNoiseDraw);
#pragma unroll
            for (int i = 0; i < I; ++i) {
                const DebandOffset o = deband_offset(deband_r(r0, (uint32_t)(i + 1)), radius * (i + 1));
#pragma unroll
                for (int t = 0; t < kDebandTaps; ++t) {
                    const DebandOffset d = deband_tap(o, t);
                    const uint32_t tx = deband_clamped(x + p, d.x, W), ty = deband_clamped(y, d.y, H);
                    taps[p][kDebandTaps * i + t] = *reinterpret_cast<const uint32_t *>(in + (size_t)ty * inPitch + (size_t)tx * 4u);
                }
            }
        }

        uint32_t px[kPixels];
#pragma unroll
        for (uint32_t p = 0; p < kPixels; ++p) px[p] = deband_texel<I>(c[p], taps[p], threshold, grain, noise[p]);
        uint8_t *__restrict__ o = outRow + (size_t)x * 4u;
        if constexpr (kWide) store_16_guarded(o, uint4{px[0], px[1], px[2], px[3]});
        else *reinterpret_cast<uint32_t *>(o) = px[0];
    }
}

// What lfg_deband launches, as plain C++: the dword kernel over everything, or -- base and pitch of both frames multiples of
// 16 -- the 16-byte kernel over the columns up to the last multiple of 4 and the dword kernel over the 1 .. 3 that remain.
// The parts write disjoint bytes and read only `in`, whose taps they clamp to the whole frame, not to their own columns.
struct DebandPart { bool wide; uint32_t xFirst, itemsX, gridX, gridY; };

inline DebandPart deband_part(bool wide, uint32_t xFirst, uint32_t cols, uint32_t H) {
    const uint32_t itemsX = wide ? cols / 4u : cols;
    const unsigned long long groupsX = ((unsigned long long)itemsX + kDebandWaveItems - 1u) / kDebandWaveItems;
    const unsigned long long rowGroups = ((unsigned long long)H + kDebandGroupRows - 1u) / kDebandGroupRows;      // <= 2^30
    return DebandPart{wide, xFirst, itemsX, (uint32_t)rowGroups, (uint32_t)(groupsX < kDebandMaxGridY ? groupsX : kDebandMaxGridY)};
}

inline int deband_parts(const void *in, size_t inPitch, const void *out, size_t outPitch, uint32_t W, uint32_t H, DebandPart (&parts)[2]) {
    const uint32_t wideW = wide_columns(multiples_of_16(in, out, inPitch, outPitch), W);
    int n = 0;
    if (wideW != 0u) parts[n++] = deband_part(true, 0u, wideW, H);
    if (wideW != W) parts[n++] = deband_part(false, wideW, W - wideW, H);
    return n;
}

template <bool kWide>
auto deband_kernel_for(int iterations) {
    return iterations == 1 ? deband_kernel<1, kWide> : iterations == 2 ? deband_kernel<2, kWide>
         : iterations == 3 ? deband_kernel<3, kWide> : deband_kernel<4, kWide>;
}

}  // namespace

hipError_t launch_deband(hipStream_t s, const lfg_frame &in, const lfg_frame &out, int iterations, int threshold, int radius, int grain,
                         uint32_t seed) {
    DebandPart parts[2];
    const int n = deband_parts(in.data, in.pitch, out.data, out.pitch, in.width, in.height, parts);
    for (int i = 0; i < n; ++i) {
        const DebandPart &p = parts[i];
        hipLaunchKernelGGL(p.wide ? deband_kernel_for<true>(iterations) : deband_kernel_for<false>(iterations), dim3(p.gridX, p.gridY),
                           dim3(kDebandWaveItems, kDebandGroupRows), 0, s, (const uint8_t *)in.data, in.pitch, (uint8_t *)out.data, out.pitch,
                           in.width, in.height, p.xFirst, p.itemsX, threshold, radius, grain, deband_seed_key(seed));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace lfg
