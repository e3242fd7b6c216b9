// upscale_edge.hip -- edge-adaptive upscaling of an RGBA8 frame (lfg_upscale_edge, include/linuxfg_hip.h, which has the
// definition).  No reference counterpart; opt-in, beside lfg_resample: a host calls it where it calls that.
// tests/edge_model.py restates the definition on the CPU.
//
// upscale_edge_kernel  per output pixel the direction and the strength of the local luma gradient over the 2 x 2 bracket, then
//                  twelve taps under a window stretched along the edge and narrowed across it, normalised by an exact
//                  division and held to the bracket's range.  The tile and both phase bodies are csrc/lfg_upscale_edge.hpp,
//                  which the CPU runs as well (tests/cpp/upscale_edge_on_host.cpp).
//
//   * A workgroup of 256 threads owns 64 x 16 output pixels.  Phase 1 stages the texels the tile's taps can reach (at most
//     67 x 19 dwords) and the per-texel analysis of the texels its brackets can be (at most 65 x 17 words of 8 bytes) into LDS:
//     13.6 KiB, static.  One barrier; phase 2 is per pixel and touches LDS and the shape table only.
//   * Integer arithmetic only, except the one float reciprocal per pixel behind the four quotients, each corrected to the
//     exact floor (edge_quotient).  Every multiply is a 24-bit one.
//   * The direction is a branch-free walk over the 16 candidates; "flat" is a select.  No data-dependent branch: the cost does
//     not depend on the content.
//   * The shape table (528 rows of 16 bytes) is read from global memory: one 16-byte load per pixel at an address that
//     depends on the content, served by the L1 -- the whole table is 8.25 KiB.
//   * A wave is 64 consecutive pixels of one output row (the row group is wave-uniform): the row's base and fraction are scalar
//     loads, LDS reads of a wave fall on one LDS row at non-decreasing columns (the same or the next dword from lane to lane:
//     no bank conflict), and a wave stores 256 contiguous bytes.  Nothing here is wider than 8 bytes on the store side.
//   * Grid: x counts tiles of 64 columns, y tiles of 16 rows (past 65,535 of them a workgroup walks on by gridDim.y).
//   * Every coordinate is clamped in phase 1, where it is read; byte offsets are size_t.
//
// Traffic: 4 bytes per input and per output pixel; the ring of a tile and the analysis' neighbours come from the caches.
// DESIGN.md section 4.25.
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_upscale_edge.hpp"

namespace lfg {
namespace {

constexpr uint32_t kEdgeMaxGridY = 65535u;

__global__ __launch_bounds__(kEdgeThreads) void upscale_edge_kernel(EdgeArgs a, uint32_t tilesY) {
    __shared__ EdgeLds edge_lds;
    const uint32_t c = threadIdx.x % kEdgeColumns;
    // the row group is the same for the 64 lanes of a wave, which the compiler cannot know: said here, the rows a wave stages
    // and the base and fraction of the output row it forms are scalar
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kEdgeColumns));
    for (uint32_t tileY = blockIdx.y; tileY < tilesY; tileY += gridDim.y) {
        edge_phase1(a, blockIdx.x, tileY, c, g, &edge_lds);
        __syncthreads();
        edge_phase2(a, blockIdx.x, tileY, c, g, &edge_lds);
        if (tileY + gridDim.y < tilesY) __syncthreads();                 // (uniform) the next tile overwrites the LDS
    }
}

}  // namespace

hipError_t launch_upscale_edge(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const EdgeAxis &x, const EdgeAxis &y,
                               const EdgeShape *shapes) {
    EdgeArgs a;
    a.in = (const uint8_t *)in.data; a.inPitch = (size_t)in.pitch;
    a.out = (uint8_t *)out.data; a.outPitch = (size_t)out.pitch;
    a.inW = in.width; a.inH = in.height;
    a.outW = out.width; a.outH = out.height;
    a.x = x; a.y = y;
    a.shapes = shapes;
    const uint32_t tilesX = (out.width - 1u) / kEdgeColumns + 1u;
    const uint32_t tilesY = (out.height - 1u) / kEdgeRows + 1u;
    hipLaunchKernelGGL(upscale_edge_kernel, dim3(tilesX, tilesY < kEdgeMaxGridY ? tilesY : kEdgeMaxGridY), dim3(kEdgeThreads), 0, s, a, tilesY);
    return hipGetLastError();
}

}  // namespace lfg
