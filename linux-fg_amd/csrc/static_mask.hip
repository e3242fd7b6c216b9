// static_mask.hip -- which pixels of a pair did not change (lfg_static_mask, include/linuxfg_hip.h): the mask that
// lfg_interpolate_compensated_masked takes.  No reference counterpart; opt-in.  tests/overlay_model.py restates it in numpy.
//
// static_mask_kernel  a thread takes four adjacent pixels of one row: one v_sad_u8 per pixel against the tolerance, and the four
//                     mask bytes leave as one dword where the mask's row puts them on a 4-byte boundary, as four bytes
//                     otherwise.  kWide -- chosen by the host when the base and the pitch of BOTH frames are multiples of 16
//                     (lfg_record_plan.hpp: multiples_of_16) -- loads the four texels of a frame with one 16-byte load, otherwise
//                     with four dword loads.  The last 1 .. 3 columns of a width that is no multiple of 4 go pixel by pixel on either path.
// No store wider than 4 bytes.  Integer arithmetic only.
//
// Traffic per pixel: 4 (prev) + 4 (curr) + 1 (mask) = 9 bytes, 75 MB at 4K.
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_record_plan.hpp"

namespace lfg {
namespace {

constexpr int kMaskBlockX = 64, kMaskBlockY = 4;   // a wave is 256 pixels of one row
constexpr int kMaskPixels = 4;                     // per thread

__device__ __forceinline__ uint32_t static_byte(uint32_t p, uint32_t c, uint32_t tolerance) {
    return __builtin_amdgcn_sad_u8(p, c, 0u) <= tolerance ? 0xffu : 0u;
}

template <bool kWide>
__global__ __launch_bounds__(kMaskBlockX * kMaskBlockY) void static_mask_kernel(
        const uint8_t *__restrict__ prev, size_t prevPitch, const uint8_t *__restrict__ curr, size_t currPitch, int W, int H,
        uint32_t tolerance, uint8_t *__restrict__ mask, size_t maskPitch) {
    const int x = (int)(blockIdx.x * kMaskBlockX + threadIdx.x) * kMaskPixels, y = (int)(blockIdx.y * kMaskBlockY + threadIdx.y);
    if (x >= W || y >= H) return;
    const uint8_t *__restrict__ p = prev + (size_t)y * prevPitch + (size_t)x * 4u;
    const uint8_t *__restrict__ c = curr + (size_t)y * currPitch + (size_t)x * 4u;
    uint8_t *__restrict__ m = mask + (size_t)y * maskPitch + (size_t)x;
    if (x + kMaskPixels > W) {                       // the last 1 .. 3 columns
        for (int i = 0; i < W - x; ++i)
            m[i] = (uint8_t)static_byte(reinterpret_cast<const uint32_t *>(p)[i], reinterpret_cast<const uint32_t *>(c)[i], tolerance);
        return;
    }
    uint32_t tp[kMaskPixels], tc[kMaskPixels];
    if (kWide) {
        const uint4 vp = *reinterpret_cast<const uint4 *>(p), vc = *reinterpret_cast<const uint4 *>(c);
        tp[0] = vp.x; tp[1] = vp.y; tp[2] = vp.z; tp[3] = vp.w;
        tc[0] = vc.x; tc[1] = vc.y; tc[2] = vc.z; tc[3] = vc.w;
    } else {
#pragma unroll
        for (int i = 0; i < kMaskPixels; ++i) {
            tp[i] = reinterpret_cast<const uint32_t *>(p)[i];
            tc[i] = reinterpret_cast<const uint32_t *>(c)[i];
        }
    }
    uint32_t word = 0u;
#pragma unroll
    for (int i = 0; i < kMaskPixels; ++i) word |= static_byte(tp[i], tc[i], tolerance) << (8 * i);
    if (((uintptr_t)m & 3u) == 0u) {
        *reinterpret_cast<uint32_t *>(m) = word;
    } else {
#pragma unroll
        for (int i = 0; i < kMaskPixels; ++i) m[i] = (uint8_t)(word >> (8 * i));
    }
}

}  // namespace

hipError_t launch_static_mask(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, int tolerance, const lfg_mask &out) {
    const int W = (int)curr.width, H = (int)curr.height;
    const bool wide = multiples_of_16(prev.data, curr.data, prev.pitch, curr.pitch);
    const int perBlock = kMaskBlockX * kMaskPixels;
    const dim3 block(kMaskBlockX, kMaskBlockY), grid((unsigned)((W + perBlock - 1) / perBlock), (unsigned)((H + kMaskBlockY - 1) / kMaskBlockY));
    const auto kernel = wide ? static_mask_kernel<true> : static_mask_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, (const uint8_t *)prev.data, (size_t)prev.pitch, (const uint8_t *)curr.data,
                       (size_t)curr.pitch, W, H, (uint32_t)tolerance, (uint8_t *)out.data, (size_t)out.pitch);
    return hipGetLastError();
}

}  // namespace lfg
