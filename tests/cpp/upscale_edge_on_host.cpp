// The kernel of csrc/upscale_edge.hip on the CPU: csrc/lfg_upscale_edge.hpp's edge_phase1 / edge_phase2 compiled with g++ alone,
// and a launch run as loops, as tests/cpp/resample_on_host.cpp runs resample_kernel: for every tile, phase 1 for all 256
// threads into a stand-in for the LDS, then (where the kernel has its barrier) phase 2 for all 256.  One case per run:
// tests/test_upscale_edge_on_host.py supplies the positions and the shape table and compares what comes out with
// tests/edge_model.py.  Frames and tables live in allocations of exactly their size, and the LDS stand-in is poisoned before
// every tile, so a build with -fsanitize=address,undefined sees every byte read or written out of range, and a word that
// phase 2 reads but phase 1 did not write shows in the bytes.
//
//   upscale_edge_on_host IN_W IN_H OUT_W OUT_H IN_PITCH OUT_PITCH LEAD_IN LEAD_OUT IN OUT POSITIONS_X POSITIONS_Y SHAPES
//
// IN holds the input rows IN_PITCH apart; OUT receives LEAD_OUT bytes, then the output rows OUT_PITCH apart, everything that is
// not a pixel 0x5A.  A positions file is base[out] (int32) then frac[out] (uint8), as lfg_upscale_edge_positions returns
// them; SHAPES is the 16 x 33 x 5 int16 of lfg_upscale_edge_shapes.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __host__
#define __device__

#include "lfg_upscale_edge.hpp"

using namespace lfg;

struct Positions {
    std::vector<int32_t> base;
    std::vector<uint8_t> frac;
    bool read(const char *path, uint32_t n) {
        base.resize(n); frac.resize(n);
        FILE *f = fopen(path, "rb");
        if (!f) return false;
        const bool ok = fread(base.data(), 4, n, f) == n && fread(frac.data(), 1, n, f) == n;
        fclose(f);
        return ok;
    }
    EdgeAxis axis() const { return EdgeAxis{base.data(), frac.data()}; }
};

int main(int argc, char **argv) {
    if (argc != 14) { fprintf(stderr, "13 arguments, see the source\n"); return 2; }
    int n = 1;
    const uint32_t inW = (uint32_t)atoi(argv[n++]), inH = (uint32_t)atoi(argv[n++]), outW = (uint32_t)atoi(argv[n++]), outH = (uint32_t)atoi(argv[n++]);
    const size_t inPitch = (size_t)atoi(argv[n++]), outPitch = (size_t)atoi(argv[n++]);
    const size_t leadIn = (size_t)atoi(argv[n++]), leadOut = (size_t)atoi(argv[n++]);
    const char *inPath = argv[n++], *outPath = argv[n++], *pxPath = argv[n++], *pyPath = argv[n++], *shapePath = argv[n++];
    Positions px, py;
    if (!px.read(pxPath, outW) || !py.read(pyPath, outH)) { fprintf(stderr, "cannot read the positions\n"); return 2; }
    constexpr size_t kRows = (size_t)kEdgeDirections * kEdgeStrengths;
    std::vector<int16_t> raw(kRows * 5);
    FILE *f = fopen(shapePath, "rb");
    if (!f || fread(raw.data(), 2, raw.size(), f) != raw.size()) { fprintf(stderr, "cannot read the shapes\n"); return 2; }
    fclose(f);
    std::vector<EdgeShape> shapes(kRows);
    for (size_t i = 0; i < kRows; ++i) shapes[i] = EdgeShape{raw[5 * i], raw[5 * i + 1], raw[5 * i + 2], raw[5 * i + 3], raw[5 * i + 4], {0, 0, 0}};

    const size_t inSize = (inH - 1) * inPitch + (size_t)inW * 4, outSize = (outH - 1) * outPitch + (size_t)outW * 4;
    uint8_t *inBase = (uint8_t *)malloc(leadIn + inSize), *outBase = (uint8_t *)malloc(leadOut + outSize);
    memset(inBase, 0x5A, leadIn + inSize);
    memset(outBase, 0x5A, leadOut + outSize);
    f = fopen(inPath, "rb");
    if (!f || fread(inBase + leadIn, 1, inSize, f) != inSize) return 2;
    fclose(f);

    EdgeArgs a;
    a.in = inBase + leadIn; a.inPitch = inPitch;
    a.out = outBase + leadOut; a.outPitch = outPitch;
    a.inW = inW; a.inH = inH; a.outW = outW; a.outH = outH;
    a.x = px.axis(); a.y = py.axis();
    a.shapes = shapes.data();
    const uint32_t tilesX = (outW - 1u) / kEdgeColumns + 1u, tilesY = (outH - 1u) / kEdgeRows + 1u;
    EdgeLds *lds = (EdgeLds *)malloc(sizeof(EdgeLds));
    for (uint32_t tileY = 0; tileY < tilesY; ++tileY)
        for (uint32_t tileX = 0; tileX < tilesX; ++tileX) {
            memset(lds, 0x7F, sizeof(EdgeLds));
            for (uint32_t t = 0; t < kEdgeThreads; ++t) edge_phase1(a, tileX, tileY, t % kEdgeColumns, t / kEdgeColumns, lds);
            for (uint32_t t = 0; t < kEdgeThreads; ++t) edge_phase2(a, tileX, tileY, t % kEdgeColumns, t / kEdgeColumns, lds);
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
