// The two kernels of csrc/sharpen.hip compiled for the CPU with g++ alone: the file is included as it is (LFG_SHARPEN_ON_HOST
// leaves out its headers and its launch function), the HIP built-ins it uses are stood in for below, and a launch is four
// nested loops over blocks and threads, for the parts that sharpen_parts -- the launch function's own arrangement -- names.
// One case per run: tests/test_sharpen_on_host.py compares what comes out with tests/sharpen_model.py.  The stand-in for the
// 16-byte store checks the range and the 16-byte alignment that the wide items promise; both frames live in allocations of
// exactly their size behind a 16-byte aligned base, so a build with -fsanitize=address,undefined also sees every byte read or
// written out of range and every misaligned wide access.
//
//   sharpen_on_host W H IN_PITCH OUT_PITCH LEAD_IN LEAD_OUT STRENGTH IN OUT
//   sharpen_on_host --rows                 prints the strip length R of the kernels
//
// IN holds the input allocation after its leading bytes (rows at IN_PITCH), OUT receives the output allocation, leading bytes
// and padding included.  Bytes nothing wrote are 0x5A.  Prints which kernels ran ("wide", "dword", "wide dword").
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define LFG_SHARPEN_ON_HOST
#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct Dim3 { unsigned x, y, z; };
static Dim3 blockIdx, threadIdx, gridDim;
struct uint4 { unsigned x, y, z, w; };
static uint8_t *g_outLo, *g_outHi;
static long g_refused = 0;
namespace lfg {
static inline void store_16_guarded(uint8_t *p, uint4 q) {
    if (p < g_outLo || p + 16 > g_outHi || (uintptr_t)p % 16) { ++g_refused; return; }
    memcpy(p, &q, 16);
}
static inline uint32_t wave_uniform(uint32_t v) { return v; }
}

#include "sharpen.hip"

using namespace lfg;

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "--rows") == 0) { printf("%d\n", kSharpenRows); return 0; }      // the strip length R
    if (argc != 10) { fprintf(stderr, "9 arguments, see the source\n"); return 2; }
    int a = 1;
    const uint32_t W = (uint32_t)atoi(argv[a++]), H = (uint32_t)atoi(argv[a++]);
    const size_t inPitch = (size_t)atoi(argv[a++]), outPitch = (size_t)atoi(argv[a++]);
    const size_t leadIn = (size_t)atoi(argv[a++]), leadOut = (size_t)atoi(argv[a++]);
    const int strength = atoi(argv[a++]);
    const char *inPath = argv[a++], *outPath = argv[a++];
    const size_t inSize = (H - 1) * inPitch + (size_t)W * 4, outSize = (H - 1) * outPitch + (size_t)W * 4;
    uint8_t *inBase = (uint8_t *)malloc(leadIn + inSize), *outBase = (uint8_t *)malloc(leadOut + outSize);       // (16-byte aligned)
    if ((uintptr_t)inBase % 16 || (uintptr_t)outBase % 16) { fprintf(stderr, "malloc gave less than 16-byte alignment\n"); return 2; }
    memset(inBase, 0x5A, leadIn + inSize);
    memset(outBase, 0x5A, leadOut + outSize);
    uint8_t *in = inBase + leadIn, *out = outBase + leadOut;
    g_outLo = out;
    g_outHi = out + outSize;
    FILE *f = fopen(inPath, "rb");
    if (!f || fread(in, 1, inSize, f) != inSize) return 2;
    fclose(f);
    SharpenPart parts[2];
    const int n = sharpen_parts(in, inPitch, out, outPitch, W, H, parts);
    for (int i = 0; i < n; ++i) {
        const SharpenPart &p = parts[i];
        gridDim = Dim3{p.gridX, p.gridY, 1};
        for (unsigned by = 0; by < p.gridY; ++by)
            for (unsigned bx = 0; bx < p.gridX; ++bx)
                for (unsigned ty = 0; ty < (unsigned)kSharpenGroupStrips; ++ty)
                    for (unsigned tx = 0; tx < (unsigned)kSharpenWaveItems; ++tx) {
                        blockIdx = Dim3{bx, by, 0};
                        threadIdx = Dim3{tx, ty, 0};
                        if (p.wide) sharpen_kernel<true>(in, inPitch, out, outPitch, W, H, p.xFirst, p.itemsX, strength);
                        else sharpen_kernel<false>(in, inPitch, out, outPitch, W, H, p.xFirst, p.itemsX, strength);
                    }
        printf("%s%s", i ? " " : "", p.wide ? "wide" : "dword");
    }
    printf("\n");
    if (g_refused) { fprintf(stderr, "%ld 16-byte stores out of range or misaligned\n", g_refused); return 3; }
    f = fopen(outPath, "wb");
    if (!f) return 2;
    fwrite(outBase, 1, leadOut + outSize, f);
    fclose(f);
    free(inBase);
    free(outBase);
    return 0;
}
