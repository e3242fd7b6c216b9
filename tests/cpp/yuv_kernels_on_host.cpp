// The two conversion kernels of csrc/yuv_convert.hip compiled for the CPU with g++ alone: the file is included as it is
// (LFG_YUV_ON_HOST leaves out its headers and its launch functions), the HIP built-ins it uses are stood in for below, and a
// launch is four nested loops over blocks and threads.  One case per run: tests/test_yuv_kernels_on_host.py compares what
// comes out with tests/yuv_model.py.  The stand-in for the 16-byte buffer store checks what the descriptor checks on the
// device (the range) and what the wide items promise (16-byte alignment); the planes live in allocations of exactly their
// size, so a build with -fsanitize=address,undefined also sees every byte out of range and every misaligned wide access.
//
//   yuv_kernels_on_host DIRECTION SITING W H Y_PITCH UV_PITCH RGBA_PITCH LEAD_Y LEAD_UV LEAD_RGBA WIDE_ITEMS IN OUT K0 .. K14
//
// DIRECTION 0: IN holds the luma plane then the chroma plane (rows at their pitches), OUT receives the RGBA allocation, leading
// bytes and padding included; 1: the other way round.  K: to_rgb[5], to_yuv[9], offset.  Bytes nothing wrote are 0x5A.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define LFG_YUV_ON_HOST
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct Dim3 { unsigned x, y, z; };
static Dim3 blockIdx, threadIdx;
struct uint2 { unsigned x, y; };
struct uint4 { unsigned x, y, z, w; };
static inline uint2 make_uint2(unsigned a, unsigned b) { return uint2{a, b}; }
enum { LFG_CHROMA_REPLICATE = 0, LFG_CHROMA_LEFT = 1 };
struct BufferResource { uint8_t *base; long bytes; };
typedef BufferResource __amdgpu_buffer_rsrc_t;
static long g_refused = 0;
static inline BufferResource __builtin_amdgcn_make_buffer_rsrc(uint8_t *p, int, int bytes, int) { return BufferResource{p, bytes}; }
struct u32x4_store { unsigned a, b, c, d; };
constexpr int kRsrcRaw32 = 0;
template <int AUX> static inline void store_b128_guarded(u32x4_store q, BufferResource r, int offset) {
    if (offset < 0 || offset + 16 > r.bytes || (uintptr_t)(r.base + offset) % 16) { ++g_refused; return; }
    memcpy(r.base + offset, &q, 16);
}
namespace lfg {
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline int kept_apart(int v) { return v; }                               // (a guard against a device code pattern: nothing to do here)
struct YuvCoefficients { int32_t to_rgb[5]; int32_t to_yuv[9]; int32_t offset; };
}

#include "yuv_convert.hip"

using namespace lfg;

int main(int argc, char **argv) {
    if (argc != 29) { fprintf(stderr, "28 arguments, see the source\n"); return 2; }
    int a = 1;
    const int direction = atoi(argv[a++]), siting = atoi(argv[a++]);
    const uint32_t W = (uint32_t)atoi(argv[a++]), H = (uint32_t)atoi(argv[a++]);
    const size_t yPitch = (size_t)atoi(argv[a++]), uvPitch = (size_t)atoi(argv[a++]), rgbaPitch = (size_t)atoi(argv[a++]);
    const size_t leadY = (size_t)atoi(argv[a++]), leadUv = (size_t)atoi(argv[a++]), leadRgba = (size_t)atoi(argv[a++]);
    const uint32_t wide = (uint32_t)atoi(argv[a++]);
    const char *in = argv[a++], *out = argv[a++];
    YuvCoefficients k;
    for (int i = 0; i < 5; ++i) k.to_rgb[i] = atoi(argv[a++]);
    for (int i = 0; i < 9; ++i) k.to_yuv[i] = atoi(argv[a++]);
    k.offset = atoi(argv[a++]);
    const size_t ySize = (H - 1) * yPitch + W, uvSize = (H / 2 - 1) * uvPitch + W, rgbaSize = (H - 1) * rgbaPitch + (size_t)W * 4;
    uint8_t *yBase = (uint8_t *)malloc(leadY + ySize), *uvBase = (uint8_t *)malloc(leadUv + uvSize), *rgbaBase = (uint8_t *)malloc(leadRgba + rgbaSize);
    memset(yBase, 0x5A, leadY + ySize);
    memset(uvBase, 0x5A, leadUv + uvSize);
    memset(rgbaBase, 0x5A, leadRgba + rgbaSize);
    uint8_t *y = yBase + leadY, *uv = uvBase + leadUv, *rgba = rgbaBase + leadRgba;
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    if (direction == 0 ? fread(y, 1, ySize, f) != ySize || fread(uv, 1, uvSize, f) != uvSize : fread(rgba, 1, rgbaSize, f) != rgbaSize) return 2;
    fclose(f);
    const uint32_t itemsX = wide + (W - 8 * wide) / 2;                          // as launch_nv12_to_rgba / launch_rgba_to_nv12
    const unsigned gridX = (itemsX + kYuvWaveItems - 1) / kYuvWaveItems, gridY = (H / 2 + kYuvGroupRows - 1) / kYuvGroupRows;
    for (unsigned by = 0; by < gridY; ++by)
        for (unsigned bx = 0; bx < gridX; ++bx)
            for (unsigned ty = 0; ty < (unsigned)kYuvGroupRows; ++ty)
                for (unsigned tx = 0; tx < (unsigned)kYuvWaveItems; ++tx) {
                    blockIdx = Dim3{bx, by, 0};
                    threadIdx = Dim3{tx, ty, 0};
                    if (direction == 0 && siting == LFG_CHROMA_LEFT) nv12_to_rgba_kernel<LFG_CHROMA_LEFT>(y, yPitch, uv, uvPitch, rgba, rgbaPitch, W, H, wide, itemsX, k);
                    else if (direction == 0) nv12_to_rgba_kernel<LFG_CHROMA_REPLICATE>(y, yPitch, uv, uvPitch, rgba, rgbaPitch, W, H, wide, itemsX, k);
                    else if (siting == LFG_CHROMA_LEFT) rgba_to_nv12_kernel<LFG_CHROMA_LEFT>(rgba, rgbaPitch, y, yPitch, uv, uvPitch, W, H, wide, itemsX, k);
                    else rgba_to_nv12_kernel<LFG_CHROMA_REPLICATE>(rgba, rgbaPitch, y, yPitch, uv, uvPitch, W, H, wide, itemsX, k);
                }
    if (g_refused) { fprintf(stderr, "%ld 16-byte stores out of range or misaligned\n", g_refused); return 3; }
    f = fopen(out, "wb");
    if (!f) return 2;
    if (direction == 0) fwrite(rgbaBase, 1, leadRgba + rgbaSize, f);
    else { fwrite(yBase, 1, leadY + ySize, f); fwrite(uvBase, 1, leadUv + uvSize, f); }
    fclose(f);
    free(yBase); free(uvBase); free(rgbaBase);
    return 0;
}
