// resample_light.hip -- lfg_resample with its sums formed in linear or in sigmoidal light instead of on the sRGB-encoded bytes
// (lfg_resample_light, include/linuxfg_hip.h).  No reference counterpart.  tests/light_model.py restates the definition on the CPU.
//
// resample_light_kernel  resample_kernel (resample.hip) with two tables between the bytes and the sums: the tile plan, the LDS
//                  row layout, the grid and the thread roles are the same, and the bodies are csrc/lfg_resample.hpp's
//                  resample_light_stage / _phase1 / _phase2, which the CPU runs as well (tests/cpp/light_on_host.cpp).
//
//   * forward[256] takes a colour byte to 14 bits of light, threshold[255] takes 14 bits back to the byte (lfg_light_tables:
//     the mode is nothing but the tables' content, so linear and sigmoidal light are one kernel).  Alpha is not light and keeps
//     resample_kernel's arithmetic.  Integers only past the tables: the bytes are a CPU model's.
//   * Both tables live in LDS behind the tile's rows, packed as uint16_t: span * 512 + 1024 bytes per launch.  A workgroup
//     stages them once, one dword per thread, before its loop over tiles, behind one more barrier.
//   * Phase 1 looks each colour byte up per tap: three ds_read_u16 per tap and row at addresses the content picks.  Four
//     entries share a bank, so 32 lanes with unrelated bytes conflict a few ways; lanes with the same byte broadcast.  The
//     alternative -- linearising the tile's source texels once into LDS and filtering from there -- is not built (DESIGN.md
//     section 4.29).
//   * Phase 2 ends a colour channel with an eight-step search of threshold[] (pos += s where threshold[pos + s - 1] <= L,
//     s = 128 .. 1): eight dependent ds_read_u16 and selects, no branch.  The cost does not depend on the content.
//   * Alpha's clamp to a byte goes through resample_byte (resample_kept_apart); the colour bytes are search positions, not
//     clamped shifts.  The build refuses the folded shift-clamp-pack instruction (check_store_hazard.py).
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_resample.hpp"

namespace lfg {
namespace {

constexpr uint32_t kResampleMaxGridY = 65535u;

__global__ __launch_bounds__(kResampleThreads) void resample_light_kernel(ResampleLightArgs a, uint32_t tilesY) {
    extern __shared__ ResampleWord resample_light_lds[];
    const uint32_t c = threadIdx.x % kResampleColumns;
    // (as in resample_kernel) the row group is wave-uniform, which the compiler cannot know
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kResampleColumns));
    resample_light_stage(a, threadIdx.x, resample_light_lds);
    __syncthreads();
    for (uint32_t tileY = blockIdx.y; tileY < tilesY; tileY += gridDim.y) {
        resample_light_phase1(a, blockIdx.x, tileY, c, g, resample_light_lds);
        __syncthreads();
        resample_light_phase2(a, blockIdx.x, tileY, c, g, resample_light_lds);
        if (tileY + gridDim.y < tilesY) __syncthreads();                 // (uniform) the next tile overwrites the rows
    }
}

}  // namespace

hipError_t launch_resample_light(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const ResampleAxis &x, const ResampleAxis &y,
                                 const ResamplePlan &plan, const uint32_t *tables) {
    ResampleLightArgs a;
    a.r.in = (const uint8_t *)in.data; a.r.inPitch = (size_t)in.pitch;
    a.r.out = (uint8_t *)out.data; a.r.outPitch = (size_t)out.pitch;
    a.r.outW = out.width; a.r.outH = out.height;
    a.r.x = x; a.r.y = y;
    a.r.rows = plan.rows;
    a.tables = tables;
    a.span = plan.span;
    const uint32_t tilesX = (out.width - 1u) / kResampleColumns + 1u;
    const uint32_t tilesY = (out.height - 1u) / plan.rows + 1u;
    const size_t lds = (size_t)plan.span * kResampleColumns * sizeof(ResampleWord) + kLightTableBytes;
    hipLaunchKernelGGL(resample_light_kernel, dim3(tilesX, tilesY < kResampleMaxGridY ? tilesY : kResampleMaxGridY), dim3(kResampleThreads), lds, s, a,
                       tilesY);
    return hipGetLastError();
}

}  // namespace lfg
