// resample.hip -- resampling of an RGBA8 frame with a choice of filter, anti-aliased where an axis shrinks (lfg_resample,
// include/linuxfg_hip.h).  No reference counterpart; lfg_scale and scale.hip stay what the reference's shader is.
// tests/resample_model.py restates the definition on the CPU.
//
// resample_kernel  ONE launch for both passes: a workgroup of 256 threads owns 64 output columns x T output rows, forms the
//                  horizontal pass of the source rows its tile needs into LDS (four int16 per row and column, 8 bytes), and
//                  after one barrier the vertical pass from there.  The intermediate image never exists in memory: through
//                  memory it would be 8 bytes per (input row, output column), 66 MB at 1080p -> 4K next to the 41 MB the call
//                  has to move.  The tile plan and both phase bodies are csrc/lfg_resample.hpp, which the CPU runs as well
//                  (tests/cpp/resample_on_host.cpp).
//
//   * Integer arithmetic only: weights are int16 with 14 fractional bits, every row of a table sums to 16384 exactly, the
//     horizontal sums are exact in 32 bits, h' keeps 6 fractional bits in 16.  No data-dependent branch: the cost does
//     not depend on the content.
//   * The table (lfg_resample_taps, built once per (filter, in, out) and kept by the context) already has the edge
//     replication folded in: first >= 0 and first + count <= in, so the kernel never clamps a coordinate.
//   * T is the host's choice per call -- the largest of 16, 8, 4, 2, 1 at which the rows of every tile fit 64 LDS rows
//     (resample_plan) -- and the launch asks for span * 512 bytes of LDS, the most rows a tile of that plan needs: an upscale
//     takes 5 to 11 KiB, a steep downscale the whole 32 KiB.
//   * Grid: x counts tiles of 64 columns, y tiles of T rows (past 65,535 of them a workgroup walks on by gridDim.y).
//   * Stores are dwords (a wave: 256 contiguous bytes), loads dwords: nothing here is wider than 8 bytes.
//
// Traffic: 4 bytes per input and per output pixel, plus the source rows that neighbouring tiles both need (the taps of a
// tile's first and last rows), which come from L2.  DESIGN.md section 4.16.
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_resample.hpp"

namespace lfg {
namespace {

constexpr uint32_t kResampleMaxGridY = 65535u;

__global__ __launch_bounds__(kResampleThreads) void resample_kernel(ResampleArgs a, uint32_t tilesY) {
    extern __shared__ ResampleWord resample_lds[];
    const uint32_t c = threadIdx.x % kResampleColumns;
    // the row group is the same for the 64 lanes of a wave, which the compiler cannot know: said here, a row's first tap, its
    // count and its weights are scalar loads in phase 2
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kResampleColumns));
    for (uint32_t tileY = blockIdx.y; tileY < tilesY; tileY += gridDim.y) {
        resample_phase1(a, blockIdx.x, tileY, c, g, resample_lds);
        __syncthreads();
        resample_phase2(a, blockIdx.x, tileY, c, g, resample_lds);
        if (tileY + gridDim.y < tilesY) __syncthreads();                 // (uniform) the next tile overwrites the rows
    }
}

}  // namespace

hipError_t launch_resample(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const ResampleAxis &x, const ResampleAxis &y,
                           const ResamplePlan &plan) {
    ResampleArgs a;
    a.in = (const uint8_t *)in.data; a.inPitch = (size_t)in.pitch;
    a.out = (uint8_t *)out.data; a.outPitch = (size_t)out.pitch;
    a.outW = out.width; a.outH = out.height;
    a.x = x; a.y = y;
    a.rows = plan.rows;
    const uint32_t tilesX = (out.width - 1u) / kResampleColumns + 1u;
    const uint32_t tilesY = (out.height - 1u) / plan.rows + 1u;
    const size_t lds = (size_t)plan.span * kResampleColumns * sizeof(ResampleWord);
    hipLaunchKernelGGL(resample_kernel, dim3(tilesX, tilesY < kResampleMaxGridY ? tilesY : kResampleMaxGridY), dim3(kResampleThreads), lds, s, a, tilesY);
    return hipGetLastError();
}

}  // namespace lfg
