// The window-cost family and the denoiser on the CPU through tests/cpp/hip_on_host: motion_refine.hip, motion_expand.hip,
// motion_subpel.hip and denoise.hip compiled by g++ as they are, and their own launch_* functions run on buffers that end where
// their last row ends (tests/cpp/on_host_frames.hpp).  tests/test_window_cost_on_host.py holds every output to the stage's CPU
// model.  One case per line of the manifest:
//
//   refine   W H radius                prev curr mvIn mvOut
//   expand   W H radius                prev curr mvLow mvOut          mvLow is ceil(W / 2) x ceil(H / 2)
//   halve    W H                       in out                         out is ceil(W / 2) x ceil(H / 2)
//   subpel   W H radius                prev curr mvIn mvqOut
//   denoise  W H count radius tolerance strength limit  curr ref0 mv0 [ref1 mv1] out
//
// motion_refine and motion_expand stage a tile in LDS behind a barrier: their launches give every lane a thread (and are what
// the -fsanitize=thread build is for); the others are plain loops over the lanes.
#include "lfg_internal.hpp"
#include "on_host_frames.hpp"

using namespace on_host;

static void must(hipError_t e) { if (e != hipSuccess) die("a launcher returned an error"); }

int main(int argc, char **argv) {
    return run_manifest(argc, argv, [](const std::vector<std::string> &a) {
        const std::string &op = a[0];
        size_t i = 1;
        auto integer = [&] { return std::stoi(a.at(i++)); };
        auto word = [&]() -> const std::string & { return a.at(i++); };
        const int W = integer(), H = integer();
        const int WL = (W + 1) / 2, HL = (H + 1) / 2;
        const uint32_t RGBA = LFG_FORMAT_RGBA8_UNORM, MV = LFG_FORMAT_MV_S8X2;
        if (op == "refine" || op == "expand" || op == "subpel") {
            const int radius = integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true);
            Buffer in = op == "expand" ? vectors(word(), WL, HL, true) : vectors(word(), W, H, true);
            Buffer out = op == "subpel" ? rgba(word(), W, H, false) : vectors(word(), W, H, false);
            hip_on_host::LaneThreads threads(op != "subpel");
            if (op == "refine") must(lfg::launch_motion_refine(nullptr, prev.frame(W, RGBA), curr.frame(W, RGBA), in.frame(W, MV), out.frame(W, MV), radius));
            else if (op == "expand") must(lfg::launch_motion_expand(nullptr, prev.frame(W, RGBA), curr.frame(W, RGBA), in.frame(WL, MV), out.frame(W, MV), radius));
            else must(lfg::launch_motion_subpel(nullptr, prev.frame(W, RGBA), curr.frame(W, RGBA), in.frame(W, MV), out.frame(W, LFG_FORMAT_MV_S16X2_Q2), radius));
            out.write();
        } else if (op == "halve") {
            Buffer in = rgba(word(), W, H, true), out = rgba(word(), WL, HL, false);
            must(lfg::launch_frame_halve(nullptr, in.frame(W, RGBA), out.frame(WL, RGBA)));
            out.write();
        } else if (op == "denoise") {
            const int count = integer(), radius = integer(), tolerance = integer(), strength = integer(), limit = integer();
            Buffer curr = rgba(word(), W, H, true);
            Buffer ref[2], mv[2];
            lfg_frame refFrame[2], mvFrame[2];
            const lfg_frame *refs[2], *mvs[2];
            for (int k = 0; k < count; ++k) {
                ref[k] = rgba(word(), W, H, true);
                mv[k] = vectors(word(), W, H, true);
                refFrame[k] = ref[k].frame(W, RGBA); mvFrame[k] = mv[k].frame(W, MV);
                refs[k] = &refFrame[k]; mvs[k] = &mvFrame[k];
            }
            Buffer out = rgba(word(), W, H, false);
            must(lfg::launch_denoise_temporal(nullptr, curr.frame(W, RGBA), refs, mvs, count, out.frame(W, RGBA), radius, tolerance, strength, limit));
            out.write();
        } else {
            die("unknown case " + op);
        }
    });
}
