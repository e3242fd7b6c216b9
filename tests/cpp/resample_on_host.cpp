// The kernel of csrc/resample.hip on the CPU: csrc/lfg_resample.hpp -- the tile plan and the two phase bodies that the kernel
// is made of -- compiled with g++ alone, and a launch run as loops: for every tile, phase 1 for all 256 threads into a stand-in
// for the LDS, then (where the kernel has its barrier) phase 2 for all 256.  One case per run: tests/test_resample_on_host.py
// supplies the tables and compares what comes out with tests/resample_model.py.  Both frames live in allocations of exactly
// their size and the LDS stand-in has exactly the plan's span of rows, poisoned before every tile, so a build with
// -fsanitize=address,undefined sees every byte read or written out of range, and a row that phase 2 reads but phase 1 did not
// write shows in the bytes.
//
//   resample_on_host IN_W IN_H OUT_W OUT_H IN_PITCH OUT_PITCH LEAD_IN LEAD_OUT IN OUT TABLE_X TABLE_Y
//
// IN holds the input allocation after its leading bytes (rows at IN_PITCH), OUT receives the output allocation, leading bytes
// and padding included; bytes nothing wrote are 0x5A.  A TABLE file is first[out] (int32), count[out] (uint32) and
// weights[out][64] (int16), as lfg_resample_taps returns them.  Prints the plan: "T span".
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __host__
#define __device__

#include "lfg_resample.hpp"

using namespace lfg;

struct Table {
    std::vector<int32_t> first;
    std::vector<uint32_t> count;
    std::vector<int16_t> weights;
    bool read(const char *path, uint32_t n) {
        first.resize(n); count.resize(n); weights.resize((size_t)n * 64);
        FILE *f = fopen(path, "rb");
        if (!f) return false;
        const bool ok = fread(first.data(), 4, n, f) == n && fread(count.data(), 4, n, f) == n && fread(weights.data(), 2, (size_t)n * 64, f) == (size_t)n * 64;
        fclose(f);
        return ok;
    }
    ResampleAxis axis() const { return ResampleAxis{first.data(), count.data(), weights.data(), 64u}; }
};

int main(int argc, char **argv) {
    if (argc != 13) { fprintf(stderr, "12 arguments, see the source\n"); return 2; }
    int n = 1;
    const uint32_t inW = (uint32_t)atoi(argv[n++]), inH = (uint32_t)atoi(argv[n++]), outW = (uint32_t)atoi(argv[n++]), outH = (uint32_t)atoi(argv[n++]);
    const size_t inPitch = (size_t)atoi(argv[n++]), outPitch = (size_t)atoi(argv[n++]);
    const size_t leadIn = (size_t)atoi(argv[n++]), leadOut = (size_t)atoi(argv[n++]);
    const char *inPath = argv[n++], *outPath = argv[n++], *txPath = argv[n++], *tyPath = argv[n++];
    Table tx, ty;
    if (!tx.read(txPath, outW) || !ty.read(tyPath, outH)) { fprintf(stderr, "cannot read a table\n"); return 2; }
    const size_t inSize = (inH - 1) * inPitch + (size_t)inW * 4, outSize = (outH - 1) * outPitch + (size_t)outW * 4;
    uint8_t *inBase = (uint8_t *)malloc(leadIn + inSize), *outBase = (uint8_t *)malloc(leadOut + outSize);
    memset(inBase, 0x5A, leadIn + inSize);
    memset(outBase, 0x5A, leadOut + outSize);
    FILE *f = fopen(inPath, "rb");
    if (!f || fread(inBase + leadIn, 1, inSize, f) != inSize) return 2;
    fclose(f);

    const ResamplePlan plan = resample_plan(ty.first.data(), ty.count.data(), outH);
    printf("%u %u\n", plan.rows, plan.span);
    ResampleArgs a;
    a.in = inBase + leadIn; a.inPitch = inPitch;
    a.out = outBase + leadOut; a.outPitch = outPitch;
    a.outW = outW; a.outH = outH;
    a.x = tx.axis(); a.y = ty.axis();
    a.rows = plan.rows;
    const uint32_t tilesX = (outW - 1u) / kResampleColumns + 1u, tilesY = (outH - 1u) / plan.rows + 1u;
    ResampleWord *lds = (ResampleWord *)malloc((size_t)plan.span * kResampleColumns * sizeof(ResampleWord));   // exactly what the launch asks for
    for (uint32_t by = 0; by < tilesY; ++by)
        for (uint32_t bx = 0; bx < tilesX; ++bx) {
            memset(lds, 0x7F, (size_t)plan.span * kResampleColumns * sizeof(ResampleWord));
            for (uint32_t t = 0; t < kResampleThreads; ++t) resample_phase1(a, bx, by, t % kResampleColumns, t / kResampleColumns, lds);
            for (uint32_t t = 0; t < kResampleThreads; ++t) resample_phase2(a, bx, by, t % kResampleColumns, t / kResampleColumns, lds);
        }
    f = fopen(outPath, "wb");
    if (!f) return 2;
    fwrite(outBase, 1, leadOut + outSize, f);
    fclose(f);
    free(lds);
    free(inBase);
    free(outBase);
    return 0;
}
