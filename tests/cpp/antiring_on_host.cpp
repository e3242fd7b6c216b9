// The kernel of csrc/resample_antiring.hip on the CPU: csrc/lfg_resample.hpp's resample_antiring_phase1 / _phase2 compiled with
// g++ alone, and a launch run as loops, as tests/cpp/resample_on_host.cpp runs resample_kernel: for every tile, phase 1 for all
// 256 threads into a stand-in for the LDS, then (where the kernel has its barrier) phase 2 for all 256.  One case per run:
// tests/test_antiring_on_host.py supplies the tables and the brackets and compares what comes out with tests/antiring_model.py.
// Frames, tables and brackets live in allocations of exactly their size and the LDS stand-in has exactly the plan's span of
// rows, poisoned before every tile, so a build with -fsanitize=address,undefined sees every byte read or written out of range
// -- a bracket outside the taps' rows among them -- and a row that phase 2 reads but phase 1 did not write shows in the bytes.
//
//   antiring_on_host IN_W IN_H OUT_W OUT_H IN_PITCH OUT_PITCH LEAD_IN LEAD_OUT IN OUT TABLE_X TABLE_Y SX SY BRACKET_X BRACKET_Y
//
// As resample_on_host, then the strength of the horizontal and of the vertical pass and a file of lo[out], hi[out] (int32) per
// axis, as lfg_resample_brackets returns them; the file of a pass whose strength is 0 is not opened ("-").  Prints the plan: "T span".
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

struct Bracket {
    std::vector<int32_t> lo, hi;
    bool read(const char *path, uint32_t n, int strength) {
        if (!strength) return true;                                // not read by the phases either: the pointers stay null
        lo.resize(n); hi.resize(n);
        FILE *f = fopen(path, "rb");
        if (!f) return false;
        const bool ok = fread(lo.data(), 4, n, f) == n && fread(hi.data(), 4, n, f) == n;
        fclose(f);
        return ok;
    }
    ResampleBracket bracket() const { return lo.empty() ? ResampleBracket{nullptr, nullptr} : ResampleBracket{lo.data(), hi.data()}; }
};

int main(int argc, char **argv) {
    if (argc != 17) { fprintf(stderr, "16 arguments, see the source\n"); return 2; }
    int n = 1;
    const uint32_t inW = (uint32_t)atoi(argv[n++]), inH = (uint32_t)atoi(argv[n++]), outW = (uint32_t)atoi(argv[n++]), outH = (uint32_t)atoi(argv[n++]);
    const size_t inPitch = (size_t)atoi(argv[n++]), outPitch = (size_t)atoi(argv[n++]);
    const size_t leadIn = (size_t)atoi(argv[n++]), leadOut = (size_t)atoi(argv[n++]);
    const char *inPath = argv[n++], *outPath = argv[n++], *txPath = argv[n++], *tyPath = argv[n++];
    const int sx = atoi(argv[n++]), sy = atoi(argv[n++]);
    const char *bxPath = argv[n++], *byPath = argv[n++];
    Table tx, ty;
    Bracket bx, by;
    if (!tx.read(txPath, outW) || !ty.read(tyPath, outH)) { fprintf(stderr, "cannot read a table\n"); return 2; }
    if (!bx.read(bxPath, outW, sx) || !by.read(byPath, outH, sy)) { fprintf(stderr, "cannot read a bracket\n"); return 2; }
    const size_t inSize = (inH - 1) * inPitch + (size_t)inW * 4, outSize = (outH - 1) * outPitch + (size_t)outW * 4;
    uint8_t *inBase = (uint8_t *)malloc(leadIn + inSize), *outBase = (uint8_t *)malloc(leadOut + outSize);
    memset(inBase, 0x5A, leadIn + inSize);
    memset(outBase, 0x5A, leadOut + outSize);
    FILE *f = fopen(inPath, "rb");
    if (!f || fread(inBase + leadIn, 1, inSize, f) != inSize) return 2;
    fclose(f);

    const ResamplePlan plan = resample_plan(ty.first.data(), ty.count.data(), outH);
    printf("%u %u\n", plan.rows, plan.span);
    ResampleAntiringArgs a;
    a.r.in = inBase + leadIn; a.r.inPitch = inPitch;
    a.r.out = outBase + leadOut; a.r.outPitch = outPitch;
    a.r.outW = outW; a.r.outH = outH;
    a.r.x = tx.axis(); a.r.y = ty.axis();
    a.r.rows = plan.rows;
    a.bx = bx.bracket(); a.by = by.bracket();
    a.sx = sx; a.sy = sy;
    const uint32_t tilesX = (outW - 1u) / kResampleColumns + 1u, tilesY = (outH - 1u) / plan.rows + 1u;
    ResampleWord *lds = (ResampleWord *)malloc((size_t)plan.span * kResampleColumns * sizeof(ResampleWord));   // exactly what the launch asks for
    for (uint32_t tileY = 0; tileY < tilesY; ++tileY)
        for (uint32_t tileX = 0; tileX < tilesX; ++tileX) {
            memset(lds, 0x7F, (size_t)plan.span * kResampleColumns * sizeof(ResampleWord));
            for (uint32_t t = 0; t < kResampleThreads; ++t) resample_antiring_phase1(a, tileX, tileY, t % kResampleColumns, t / kResampleColumns, lds);
            for (uint32_t t = 0; t < kResampleThreads; ++t) resample_antiring_phase2(a, tileX, tileY, t % kResampleColumns, t / kResampleColumns, lds);
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
