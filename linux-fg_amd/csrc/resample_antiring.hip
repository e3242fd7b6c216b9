// resample_antiring.hip -- lfg_resample with the overshoot of its upscaling passes limited (lfg_resample_antiring,
// include/linuxfg_hip.h).  No reference counterpart.  tests/antiring_model.py restates the definition on the CPU.
//
// resample_antiring_kernel  resample_kernel (resample.hip) with one addition per phase: the tile plan, the LDS layout, the
//                  grid and the launch shape are the same, and the phase bodies are csrc/lfg_resample.hpp's
//                  resample_antiring_phase1 / _phase2, which the CPU runs as well (tests/cpp/antiring_on_host.cpp).
//
//   * A 1-D pass whose axis grows may not leave the range of the two source samples that bracket the output position,
//     a(p) = floor and b(p) = ceil of the output centre in texels (lfg_resample_brackets: integers only; the tables live on
//     the device next to the axis tables).  The strength S mixes the clamped sum with the plain one in 64ths.  Integer
//     median and mix on the 32-bit sums, before either rounding: the bytes are a CPU model's, like resample_kernel's.
//   * No branch on the content and none on S.  A pass that is not anti-ringed (its axis does not grow) runs with S = 0, where
//     the mix is the identity, and reads its "bracket" at the first tap; when no pass qualifies the host launches
//     resample_kernel itself, so this kernel never runs with both strengths 0.
//   * Phase 1, the bracket texels: RELOADED -- two more dword loads per (source row, output column) -- not picked from the
//     taps' registers.  The taps arrive four to a 16-byte load inside a loop whose trip count the compiler does not know, and
//     the bracket's place among them, a(p) - first[p], differs from lane to lane.  Both were compiled.  Picking is, in the
//     ISA, a v_cndmask_b32 per tap, row and texel behind a compare per tap and texel: 32 selects in the loop of four taps and 8
//     per single tap, 48 and their compares per block of four rows under Lanczos-3's six taps, in a kernel bound by issue; it
//     needs 109 registers to the reload's 126 (both 4 waves per SIMD) and no load.  The reload is 8 global_load_dword per four
//     rows, issued ahead of the tap loop, from cache lines the tap loads of the same wave fetch anyway (a and b lie within the
//     taps), and 8 64-bit address adds.  Measured, the reload is 1 to 3 % faster at every size and filter (DESIGN.md section
//     4.22), and it is the simpler body.
//   * Phase 2, the bracket rows: a(q) and b(q) are the same for a whole wave, like the row's first tap and count, and are
//     loaded the way the compiler loads those in resample_kernel (one address for the wave); the two h' words are two more
//     ds_read_b64 at lane-consecutive addresses, conflict-free like the taps'.
//   * Every clamp to a byte goes through resample_byte (resample_kept_apart): the build refuses the folded
//     shift-clamp-pack instruction (check_store_hazard.py).
#include "lfg_internal.hpp"
#include "lfg_device.hpp"
#include "lfg_resample.hpp"

namespace lfg {
namespace {

constexpr uint32_t kResampleMaxGridY = 65535u;

__global__ __launch_bounds__(kResampleThreads) void resample_antiring_kernel(ResampleAntiringArgs a, uint32_t tilesY) {
    extern __shared__ ResampleWord resample_antiring_lds[];
    const uint32_t c = threadIdx.x % kResampleColumns;
    // (as in resample_kernel) the row group is wave-uniform, which the compiler cannot know: said here, a row's taps and its
    // bracket rows have one address for the wave in phase 2
    const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kResampleColumns));
    for (uint32_t tileY = blockIdx.y; tileY < tilesY; tileY += gridDim.y) {
        resample_antiring_phase1(a, blockIdx.x, tileY, c, g, resample_antiring_lds);
        __syncthreads();
        resample_antiring_phase2(a, blockIdx.x, tileY, c, g, resample_antiring_lds);
        if (tileY + gridDim.y < tilesY) __syncthreads();                 // (uniform) the next tile overwrites the rows
    }
}

}  // namespace

hipError_t launch_resample_antiring(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const ResampleAxis &x, const ResampleAxis &y,
                                    const ResamplePlan &plan, const ResampleBracket &bx, const ResampleBracket &by, int sx, int sy) {
    ResampleAntiringArgs a;
    a.r.in = (const uint8_t *)in.data; a.r.inPitch = (size_t)in.pitch;
    a.r.out = (uint8_t *)out.data; a.r.outPitch = (size_t)out.pitch;
    a.r.outW = out.width; a.r.outH = out.height;
    a.r.x = x; a.r.y = y;
    a.r.rows = plan.rows;
    a.bx = bx; a.by = by;
    a.sx = sx; a.sy = sy;
    const uint32_t tilesX = (out.width - 1u) / kResampleColumns + 1u;
    const uint32_t tilesY = (out.height - 1u) / plan.rows + 1u;
    const size_t lds = (size_t)plan.span * kResampleColumns * sizeof(ResampleWord);
    hipLaunchKernelGGL(resample_antiring_kernel, dim3(tilesX, tilesY < kResampleMaxGridY ? tilesY : kResampleMaxGridY), dim3(kResampleThreads), lds, s, a,
                       tilesY);
    return hipGetLastError();
}

}  // namespace lfg
