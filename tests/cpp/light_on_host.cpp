// The kernel of csrc/resample_light.hip on the CPU: csrc/lfg_resample.hpp's resample_light_stage / _phase1 / _phase2 compiled with
// g++ alone, and a launch run as loops, as tests/cpp/resample_on_host.cpp runs resample_kernel: the staging of the tables for all
// 256 threads into a stand-in for the LDS, then for every tile phase 1 for all 256 and (where the kernel has its barrier) phase 2
// for all 256.  One case per run: tests/test_light_on_host.py supplies the tables and compares what comes out with
// tests/light_model.py.  Frames and tables live in allocations of exactly their size, and the LDS stand-in has exactly what the
// launch asks for -- the plan's span of rows and the 1024 bytes of the two light tables behind them -- its rows poisoned before
// every tile, so a build with -fsanitize=address,undefined sees a lookup past a table or a row past the tile, and a row that
// phase 2 reads but phase 1 did not write shows in the bytes.
//
//   light_on_host IN_W IN_H OUT_W OUT_H IN_PITCH OUT_PITCH LEAD_IN LEAD_OUT IN OUT TABLE_X TABLE_Y LIGHT
//
// As resample_on_host, then a file of forward[256] and threshold[255], 0xFFFF (uint16) as the context uploads them.  Prints the
// plan: "T span".
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
    if (argc != 14) { fprintf(stderr, "13 arguments, see the source\n"); return 2; }
    int n = 1;
    const uint32_t inW = (uint32_t)atoi(argv[n++]), inH = (uint32_t)atoi(argv[n++]), outW = (uint32_t)atoi(argv[n++]), outH = (uint32_t)atoi(argv[n++]);
    const size_t inPitch = (size_t)atoi(argv[n++]), outPitch = (size_t)atoi(argv[n++]);
    const size_t leadIn = (size_t)atoi(argv[n++]), leadOut = (size_t)atoi(argv[n++]);
    const char *inPath = argv[n++], *outPath = argv[n++], *txPath = argv[n++], *tyPath = argv[n++], *lightPath = argv[n++];
    Table tx, ty;
    if (!tx.read(txPath, outW) || !ty.read(tyPath, outH)) { fprintf(stderr, "cannot read a table\n"); return 2; }
    uint32_t *light = (uint32_t *)malloc(kLightTableBytes);          // what the device holds: exactly 1024 bytes
    FILE *f = fopen(lightPath, "rb");
    if (!f || fread(light, 1, kLightTableBytes, f) != kLightTableBytes) { fprintf(stderr, "cannot read the light tables\n"); return 2; }
    fclose(f);
    const size_t inSize = (inH - 1) * inPitch + (size_t)inW * 4, outSize = (outH - 1) * outPitch + (size_t)outW * 4;
    uint8_t *inBase = (uint8_t *)malloc(leadIn + inSize), *outBase = (uint8_t *)malloc(leadOut + outSize);
    memset(inBase, 0x5A, leadIn + inSize);
    memset(outBase, 0x5A, leadOut + outSize);
    f = fopen(inPath, "rb");
    if (!f || fread(inBase + leadIn, 1, inSize, f) != inSize) return 2;
    fclose(f);

    const ResamplePlan plan = resample_plan(ty.first.data(), ty.count.data(), outH);
    printf("%u %u\n", plan.rows, plan.span);
    ResampleLightArgs a;
    a.r.in = inBase + leadIn; a.r.inPitch = inPitch;
    a.r.out = outBase + leadOut; a.r.outPitch = outPitch;
    a.r.outW = outW; a.r.outH = outH;
    a.r.x = tx.axis(); a.r.y = ty.axis();
    a.r.rows = plan.rows;
    a.tables = light;
    a.span = plan.span;
    const uint32_t tilesX = (outW - 1u) / kResampleColumns + 1u, tilesY = (outH - 1u) / plan.rows + 1u;
    const size_t rowBytes = (size_t)plan.span * kResampleColumns * sizeof(ResampleWord);
    ResampleWord *lds = (ResampleWord *)malloc(rowBytes + kLightTableBytes);                     // exactly what the launch asks for
    memset(lds, 0x7F, rowBytes + kLightTableBytes);
    // one workgroup per column of tiles walks its tiles, as the kernel does past 65,535 of them: the tables are staged once
    for (uint32_t tileX = 0; tileX < tilesX; ++tileX) {
        for (uint32_t t = 0; t < kResampleThreads; ++t) resample_light_stage(a, t, lds);
        for (uint32_t tileY = 0; tileY < tilesY; ++tileY) {
            memset(lds, 0x7F, rowBytes);
            for (uint32_t t = 0; t < kResampleThreads; ++t) resample_light_phase1(a, tileX, tileY, t % kResampleColumns, t / kResampleColumns, lds);
            for (uint32_t t = 0; t < kResampleThreads; ++t) resample_light_phase2(a, tileX, tileY, t % kResampleColumns, t / kResampleColumns, lds);
        }
        memset(lds, 0x7F, rowBytes + kLightTableBytes);
    }
    f = fopen(outPath, "wb");
    if (!f) return 2;
    fwrite(outBase, 1, leadOut + outSize, f);
    fclose(f);
    free(lds);
    free(light);
    free(inBase);
    free(outBase);
    return 0;
}
