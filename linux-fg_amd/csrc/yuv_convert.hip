// yuv_convert.hip -- NV12 <-> RGBA8 colour conversion (lfg_nv12_to_rgba, lfg_rgba_to_nv12, include/linuxfg_hip.h).  No
// reference counterpart; opt-in, outside the three stages.  tests/yuv_model.py restates the definition on the CPU.
//
// nv12_to_rgba_kernel  per 2 x 2 quad four luma bytes and one (Cb, Cr) pair (under LFG_CHROMA_LEFT also the pair to the right
//                      and both of the rows above and below), four RGBA texels out.  1.5 bytes read, 4 written per pixel.
// rgba_to_nv12_kernel  per quad four texels (under LFG_CHROMA_LEFT also the column to the left), four luma bytes and one pair
//                      out.  4 bytes read, 1.5 written per pixel.
//
// Both have the same shape.  A lane takes one ITEM of a pair of rows (2 j, 2 j + 1):
//   * a wide item is 8 x 2 pixels, four quads: two 8-byte luma accesses, one 8-byte chroma access, four 16-byte RGBA accesses.
//     The host offers them only when every base and pitch allows the aligned access (launch_*: kWideAlign), and then for the
//     first W / 8 items of the row pair;
//   * a narrow item is one quad through byte, 2-byte and 4-byte accesses, which the contract of the calls always allows.  The
//     0 .. 3 quads right of the last wide item are narrow items of the same launch, so no wide access is ever partial; without
//     the alignment every item is narrow.
// A wave is 64 consecutive items of one row pair -- 512 pixels of contiguous rows where the items are wide -- and a workgroup
// four such waves on four consecutive row pairs.  Every load of an item is issued before the first use of any (the loads fill
// locals that the arithmetic reads afterwards).  Matrix and range arrive as the integer coefficients of lfg_yuv_coefficients in
// a kernel argument (wave-uniform: scalar registers); the siting is a template parameter, because it decides what is loaded.
// The 16-byte stores are store_b128_guarded (lfg_device.hpp; the build checks them); nothing else stores more than 8 bytes.
// No float anywhere; every intermediate fits 32 bits.
//
// Traffic per pixel: 1.5 + 4 = 5.5 bytes in either direction, 45.6 MB at 4K.
#ifndef LFG_YUV_ON_HOST                                      // tests/cpp/yuv_kernels_on_host.cpp compiles the kernels for the CPU, with
#include "lfg_internal.hpp"                                 // its own stand-ins for what these two headers and the HIP runtime give them
#include "lfg_device.hpp"
#endif

namespace lfg {
namespace {

constexpr int kYuvWaveItems = 64;                           // items of one row pair per wave
constexpr int kYuvGroupRows = 4;                            // row pairs (waves) per workgroup
constexpr uint32_t kWideAlignPlane = 8u, kWideAlignRgba = 16u;

__device__ __forceinline__ int clamp255(int v) { return clampi(v, 0, 255); }

#ifndef LFG_YUV_ON_HOST
// hipcc (ROCm 7.2) folds two shifted values, each clamped to a byte and packed side by side, into v_ashr_pk_u8_i32 and takes
// the upper half of that instruction's result for zero; the MI355X leaves that half of the register as it was, and what was
// there went into the B byte when R, G and B were or-ed together (first seen at 2 x 2: B = 238 | 0x2d).  A value that has
// passed through here is not part of that pattern; it costs no instruction.
__device__ __forceinline__ int kept_apart(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
#endif

// The chroma of a quad's four pixels, scaled by 8, from the sample of the quad (m0), its right neighbour (m1) and the same
// two of the chroma rows above (u) and below (d), all already clamped to the plane.  Order: (even x, even y), (odd x, even y),
// (even x, odd y), (odd x, odd y).
template <int kSiting>
__device__ __forceinline__ void quad_chroma8(int m0, int m1, int u0, int u1, int d0, int d1, int (&c8)[4]) {
    if (kSiting == LFG_CHROMA_REPLICATE) {
        c8[0] = c8[1] = c8[2] = c8[3] = 8 * m0;
    } else {
        const int em = 2 * m0, om = m0 + m1, eu = 2 * u0, ou = u0 + u1, ed = 2 * d0, od = d0 + d1;
        c8[0] = 3 * em + eu;
        c8[1] = 3 * om + ou;
        c8[2] = 3 * em + ed;
        c8[3] = 3 * om + od;
    }
}

__device__ __forceinline__ uint32_t yuv_texel(int Y, int cb8, int cr8, const YuvCoefficients &k) {
    const int yy = 8 * k.to_rgb[0] * (Y - k.offset) + (1 << 16);
    const int cb = cb8 - 1024, cr = cr8 - 1024;
    const int r = kept_apart(clamp255((yy + k.to_rgb[1] * cr) >> 17));
    const int g = kept_apart(clamp255((yy - k.to_rgb[2] * cb - k.to_rgb[3] * cr) >> 17));
    const int b = kept_apart(clamp255((yy + k.to_rgb[4] * cb) >> 17));
    return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | 0xff000000u;
}

// One quad: luma l[0..3] in quad_chroma8's order, the six (Cb, Cr) pairs as 16-bit words (Cb in the low byte).
template <int kSiting>
__device__ __forceinline__ void quad_texels(const int (&l)[4], uint32_t m0, uint32_t m1, uint32_t u0, uint32_t u1, uint32_t d0,
                                            uint32_t d1, const YuvCoefficients &k, uint32_t (&px)[4]) {
    int cb8[4], cr8[4];
    quad_chroma8<kSiting>((int)(m0 & 255u), (int)(m1 & 255u), (int)(u0 & 255u), (int)(u1 & 255u), (int)(d0 & 255u), (int)(d1 & 255u), cb8);
    quad_chroma8<kSiting>((int)((m0 >> 8) & 255u), (int)((m1 >> 8) & 255u), (int)((u0 >> 8) & 255u), (int)((u1 >> 8) & 255u),
                          (int)((d0 >> 8) & 255u), (int)((d1 >> 8) & 255u), cr8);
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i] = yuv_texel(l[i], cb8[i], cr8[i], k);
}

__device__ __forceinline__ uint32_t half_of(uint2 v, int i) {                // 16-bit word i of 8 bytes
    return ((i & 2 ? v.y : v.x) >> (16 * (i & 1))) & 0xffffu;
}
__device__ __forceinline__ int byte_of(uint2 v, int i) {                     // byte i of 8 bytes
    return (int)(((i & 4 ? v.y : v.x) >> (8 * (i & 3))) & 0xffu);
}

template <int kSiting>
__global__ __launch_bounds__(kYuvWaveItems * kYuvGroupRows) void nv12_to_rgba_kernel(
        const uint8_t *__restrict__ y, size_t yPitch, const uint8_t *__restrict__ uv, size_t uvPitch, uint8_t *__restrict__ out,
        size_t outPitch, uint32_t W, uint32_t H, uint32_t wideItems, uint32_t itemsX, YuvCoefficients k) {
    const uint32_t g = blockIdx.x * (uint32_t)kYuvWaveItems + threadIdx.x;
    const uint32_t j = blockIdx.y * (uint32_t)kYuvGroupRows + threadIdx.y;
    const uint32_t cw = W / 2u, ch = H / 2u;
    if (g >= itemsX || j >= ch) return;
    constexpr bool kLeft = kSiting == LFG_CHROMA_LEFT;
    // the chroma rows above and below, clamped to the plane (read under LFG_CHROMA_LEFT only)
    const size_t rowM = (size_t)j * uvPitch, rowU = (size_t)(j > 0u ? j - 1u : 0u) * uvPitch, rowD = (size_t)(j + 1u < ch ? j + 1u : ch - 1u) * uvPitch;
    const size_t row0 = (size_t)(2u * j) * yPitch, row1 = row0 + yPitch;
    if (g < wideItems) {
        const uint32_t x0 = 8u * g, i0 = 4u * g;
        const size_t next = 2u * (size_t)(i0 + 4u < cw ? i0 + 4u : cw - 1u);       // the pair right of the item's four, clamped
        const uint2 l0 = *reinterpret_cast<const uint2 *>(y + row0 + x0);
        const uint2 l1 = *reinterpret_cast<const uint2 *>(y + row1 + x0);
        const uint2 cm = *reinterpret_cast<const uint2 *>(uv + rowM + 2u * (size_t)i0);
        uint2 cu = cm, cd = cm;
        uint32_t nm = 0u, nu = 0u, nd = 0u;
        if (kLeft) {
            cu = *reinterpret_cast<const uint2 *>(uv + rowU + 2u * (size_t)i0);
            cd = *reinterpret_cast<const uint2 *>(uv + rowD + 2u * (size_t)i0);
            nm = *reinterpret_cast<const uint16_t *>(uv + rowM + next);
            nu = *reinterpret_cast<const uint16_t *>(uv + rowU + next);
            nd = *reinterpret_cast<const uint16_t *>(uv + rowD + next);
        }
        const __amdgpu_buffer_rsrc_t rOut = __builtin_amdgcn_make_buffer_rsrc(out, 0, (int)((H - 1u) * outPitch + (size_t)W * 4u), kRsrcRaw32);
        uint32_t top[8], bottom[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int l[4] = {byte_of(l0, 2 * q), byte_of(l0, 2 * q + 1), byte_of(l1, 2 * q), byte_of(l1, 2 * q + 1)};
            uint32_t px[4];
            quad_texels<kSiting>(l, half_of(cm, q), q < 3 ? half_of(cm, q + 1) : nm, half_of(cu, q), q < 3 ? half_of(cu, q + 1) : nu,
                                 half_of(cd, q), q < 3 ? half_of(cd, q + 1) : nd, k, px);
            top[2 * q] = px[0]; top[2 * q + 1] = px[1];
            bottom[2 * q] = px[2]; bottom[2 * q + 1] = px[3];
        }
        const int o0 = (int)((size_t)(2u * j) * outPitch + (size_t)x0 * 4u), o1 = o0 + (int)outPitch;
        store_b128_guarded<0>(u32x4_store{top[0], top[1], top[2], top[3]}, rOut, o0);
        store_b128_guarded<0>(u32x4_store{top[4], top[5], top[6], top[7]}, rOut, o0 + 16);
        store_b128_guarded<0>(u32x4_store{bottom[0], bottom[1], bottom[2], bottom[3]}, rOut, o1);
        store_b128_guarded<0>(u32x4_store{bottom[4], bottom[5], bottom[6], bottom[7]}, rOut, o1 + 16);
    } else {
        const uint32_t i = 4u * wideItems + (g - wideItems), x0 = 2u * i;
        const size_t here = 2u * (size_t)i, next = 2u * (size_t)(i + 1u < cw ? i + 1u : cw - 1u);
        const int l[4] = {y[row0 + x0], y[row0 + x0 + 1u], y[row1 + x0], y[row1 + x0 + 1u]};
        const uint32_t m0 = *reinterpret_cast<const uint16_t *>(uv + rowM + here);
        uint32_t m1 = 0u, u0 = 0u, u1 = 0u, d0 = 0u, d1 = 0u;
        if (kLeft) {
            m1 = *reinterpret_cast<const uint16_t *>(uv + rowM + next);
            u0 = *reinterpret_cast<const uint16_t *>(uv + rowU + here);
            u1 = *reinterpret_cast<const uint16_t *>(uv + rowU + next);
            d0 = *reinterpret_cast<const uint16_t *>(uv + rowD + here);
            d1 = *reinterpret_cast<const uint16_t *>(uv + rowD + next);
        }
        uint32_t px[4];
        quad_texels<kSiting>(l, m0, m1, u0, u1, d0, d1, k, px);
        uint32_t *o0 = reinterpret_cast<uint32_t *>(out + (size_t)(2u * j) * outPitch + (size_t)x0 * 4u);
        uint32_t *o1 = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(o0) + outPitch);
        o0[0] = px[0]; o0[1] = px[1];
        o1[0] = px[2]; o1[1] = px[3];
    }
}

// The R, G, B of one texel, and sums of them.
struct Rgb { int r, g, b; };
__device__ __forceinline__ Rgb rgb_of(uint32_t p) { return Rgb{(int)(p & 255u), (int)((p >> 8) & 255u), (int)((p >> 16) & 255u)}; }
__device__ __forceinline__ Rgb operator+(Rgb a, Rgb b) { return Rgb{a.r + b.r, a.g + b.g, a.b + b.b}; }

__device__ __forceinline__ uint32_t luma_of(Rgb p, const YuvCoefficients &k) {
    return (uint32_t)clamp255(k.offset + ((k.to_yuv[0] * p.r + k.to_yuv[1] * p.g + k.to_yuv[2] * p.b + (1 << 13)) >> 14));
}

// The (Cb, Cr) pair of a quad as a 16-bit word, from the sums over both rows of the column left of it (l), its even (e) and
// its odd (o) column.
template <int kSiting>
__device__ __forceinline__ uint32_t pair_of(Rgb l, Rgb e, Rgb o, const YuvCoefficients &k) {
    constexpr int shift = kSiting == LFG_CHROMA_LEFT ? 17 : 16;
    Rgb s = e + o;
    if (kSiting == LFG_CHROMA_LEFT) s = s + l + e;
    const int cb = clamp255(128 + ((k.to_yuv[3] * s.r + k.to_yuv[4] * s.g + k.to_yuv[5] * s.b + (1 << (shift - 1))) >> shift));
    const int cr = clamp255(128 + ((k.to_yuv[6] * s.r + k.to_yuv[7] * s.g + k.to_yuv[8] * s.b + (1 << (shift - 1))) >> shift));
    return (uint32_t)cb | ((uint32_t)cr << 8);
}

template <int kSiting>
__global__ __launch_bounds__(kYuvWaveItems * kYuvGroupRows) void rgba_to_nv12_kernel(
        const uint8_t *__restrict__ in, size_t inPitch, uint8_t *__restrict__ y, size_t yPitch, uint8_t *__restrict__ uv, size_t uvPitch,
        uint32_t W, uint32_t H, uint32_t wideItems, uint32_t itemsX, YuvCoefficients k) {
    const uint32_t g = blockIdx.x * (uint32_t)kYuvWaveItems + threadIdx.x;
    const uint32_t j = blockIdx.y * (uint32_t)kYuvGroupRows + threadIdx.y;
    if (g >= itemsX || j >= H / 2u) return;
    constexpr bool kLeft = kSiting == LFG_CHROMA_LEFT;
    const uint8_t *__restrict__ in0 = in + (size_t)(2u * j) * inPitch, *__restrict__ in1 = in0 + inPitch;
    const size_t row0 = (size_t)(2u * j) * yPitch, row1 = row0 + yPitch, rowC = (size_t)j * uvPitch;
    if (g < wideItems) {
        const uint32_t x0 = 8u * g;
        const size_t left = 4u * (size_t)(x0 > 0u ? x0 - 1u : 0u);                 // the column left of the item, clamped
        const uint4 a0 = *reinterpret_cast<const uint4 *>(in0 + (size_t)x0 * 4u), b0 = *reinterpret_cast<const uint4 *>(in0 + (size_t)x0 * 4u + 16u);
        const uint4 a1 = *reinterpret_cast<const uint4 *>(in1 + (size_t)x0 * 4u), b1 = *reinterpret_cast<const uint4 *>(in1 + (size_t)x0 * 4u + 16u);
        uint32_t e0 = 0u, e1 = 0u;
        if (kLeft) {
            e0 = *reinterpret_cast<const uint32_t *>(in0 + left);
            e1 = *reinterpret_cast<const uint32_t *>(in1 + left);
        }
        const uint32_t t[8] = {a0.x, a0.y, a0.z, a0.w, b0.x, b0.y, b0.z, b0.w}, b[8] = {a1.x, a1.y, a1.z, a1.w, b1.x, b1.y, b1.z, b1.w};
        uint32_t lt[8], lb[8];
        Rgb col[9];                                                               // both rows summed; [0] is the column to the left
        col[0] = rgb_of(e0) + rgb_of(e1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const Rgb pt = rgb_of(t[c]), pb = rgb_of(b[c]);
            lt[c] = luma_of(pt, k);
            lb[c] = luma_of(pb, k);
            col[c + 1] = pt + pb;
        }
        uint32_t pr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pr[q] = pair_of<kSiting>(col[2 * q], col[2 * q + 1], col[2 * q + 2], k);
        *reinterpret_cast<uint2 *>(y + row0 + x0) = make_uint2(lt[0] | (lt[1] << 8) | (lt[2] << 16) | (lt[3] << 24), lt[4] | (lt[5] << 8) | (lt[6] << 16) | (lt[7] << 24));
        *reinterpret_cast<uint2 *>(y + row1 + x0) = make_uint2(lb[0] | (lb[1] << 8) | (lb[2] << 16) | (lb[3] << 24), lb[4] | (lb[5] << 8) | (lb[6] << 16) | (lb[7] << 24));
        *reinterpret_cast<uint2 *>(uv + rowC + x0) = make_uint2(pr[0] | (pr[1] << 16), pr[2] | (pr[3] << 16));
    } else {
        const uint32_t i = 4u * wideItems + (g - wideItems), x0 = 2u * i;
        const size_t left = 4u * (size_t)(x0 > 0u ? x0 - 1u : 0u);
        const uint32_t t0 = *reinterpret_cast<const uint32_t *>(in0 + (size_t)x0 * 4u), t1 = *reinterpret_cast<const uint32_t *>(in0 + (size_t)x0 * 4u + 4u);
        const uint32_t b0 = *reinterpret_cast<const uint32_t *>(in1 + (size_t)x0 * 4u), b1 = *reinterpret_cast<const uint32_t *>(in1 + (size_t)x0 * 4u + 4u);
        uint32_t e0 = 0u, e1 = 0u;
        if (kLeft) {
            e0 = *reinterpret_cast<const uint32_t *>(in0 + left);
            e1 = *reinterpret_cast<const uint32_t *>(in1 + left);
        }
        const Rgb p00 = rgb_of(t0), p01 = rgb_of(t1), p10 = rgb_of(b0), p11 = rgb_of(b1);
        const uint32_t pr = pair_of<kSiting>(rgb_of(e0) + rgb_of(e1), p00 + p10, p01 + p11, k);
        y[row0 + x0] = (uint8_t)luma_of(p00, k);
        y[row0 + x0 + 1u] = (uint8_t)luma_of(p01, k);
        y[row1 + x0] = (uint8_t)luma_of(p10, k);
        y[row1 + x0 + 1u] = (uint8_t)luma_of(p11, k);
        *reinterpret_cast<uint16_t *>(uv + rowC + 2u * (size_t)i) = (uint16_t)pr;
    }
}

#ifndef LFG_YUV_ON_HOST
// How many wide items a row pair has: W / 8 when every plane allows the aligned accesses and the RGBA frame's byte offsets fit
// the 32-bit offset of its buffer stores, else none.
uint32_t yuv_wide_items(const lfg_nv12 &p, const lfg_frame &f) {
    const bool planes = (((uintptr_t)p.y | (uintptr_t)p.uv | (uintptr_t)p.y_pitch | (uintptr_t)p.uv_pitch) % kWideAlignPlane) == 0;
    const bool rgba = (((uintptr_t)f.data | (uintptr_t)f.pitch) % kWideAlignRgba) == 0 && (uint64_t)f.height * f.pitch < 0x7fffffffull;
    return planes && rgba ? p.width / 8u : 0u;
}

#endif
}  // namespace

#ifndef LFG_YUV_ON_HOST
bool yuv_grid_ok(uint32_t width, uint32_t height) {
    return (width / 2u + kYuvWaveItems - 1u) / kYuvWaveItems <= 65535u && (height / 2u + kYuvGroupRows - 1u) / kYuvGroupRows <= 65535u;
}

hipError_t launch_nv12_to_rgba(hipStream_t s, const lfg_nv12 &in, const lfg_frame &out, const YuvCoefficients &k, int siting) {
    const uint32_t W = in.width, H = in.height, wide = yuv_wide_items(in, out), itemsX = wide + (W - 8u * wide) / 2u;
    const dim3 grid((itemsX + kYuvWaveItems - 1u) / kYuvWaveItems, (H / 2u + kYuvGroupRows - 1u) / kYuvGroupRows), block(kYuvWaveItems, kYuvGroupRows);
    const auto kernel = siting == LFG_CHROMA_LEFT ? nv12_to_rgba_kernel<LFG_CHROMA_LEFT> : nv12_to_rgba_kernel<LFG_CHROMA_REPLICATE>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, (const uint8_t *)in.y, (size_t)in.y_pitch, (const uint8_t *)in.uv, (size_t)in.uv_pitch,
                       (uint8_t *)out.data, (size_t)out.pitch, W, H, wide, itemsX, k);
    return hipGetLastError();
}

hipError_t launch_rgba_to_nv12(hipStream_t s, const lfg_frame &in, const lfg_nv12 &out, const YuvCoefficients &k, int siting) {
    const uint32_t W = out.width, H = out.height, wide = yuv_wide_items(out, in), itemsX = wide + (W - 8u * wide) / 2u;
    const dim3 grid((itemsX + kYuvWaveItems - 1u) / kYuvWaveItems, (H / 2u + kYuvGroupRows - 1u) / kYuvGroupRows), block(kYuvWaveItems, kYuvGroupRows);
    const auto kernel = siting == LFG_CHROMA_LEFT ? rgba_to_nv12_kernel<LFG_CHROMA_LEFT> : rgba_to_nv12_kernel<LFG_CHROMA_REPLICATE>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, (const uint8_t *)in.data, (size_t)in.pitch, (uint8_t *)out.y, (size_t)out.y_pitch,
                       (uint8_t *)out.uv, (size_t)out.uv_pitch, W, H, wide, itemsX, k);
    return hipGetLastError();
}
#endif

}  // namespace lfg
