// The compensated family on the CPU through tests/cpp/hip_on_host: interpolate_mc.hip, extrapolate_mc.hip, interpolate_bidir.hip,
// interpolate_subpel.hip, static_mask.hip, interpolate_bicubic.hip and hole_fill.hip compiled by g++ as they are, and their own
// launch_* functions run on buffers that end where their last row ends (tests/cpp/on_host_frames.hpp).  The key image, the
// fill plane and the 64-bit key image are allocations of exactly W * H words.  tests/test_compensated_on_host.py holds every
// output to the stage's CPU model.  One case per line of the manifest:
//
//   mc              W H t matchSad reach  prev curr mv out             reach 0: the hole walk, else the fill plane
//   masked          W H t matchSad reach  prev curr mv mask out
//   extrapolate     W H ahead matchSad    prev curr mv out
//   bidir           W H t matchSad tolerance reach  prev curr fwd bwd out
//   consistency     W H tolerance         a b mask
//   static_mask     W H tolerance         prev curr mask
//   subpel          W H t matchSad        prev curr mvq out
//   bicubic         W H t matchSad        prev curr mv out
//   subpel_bicubic  W H t matchSad        prev curr mvq out
//   fill_plane      W H reach passStatic band  keys plane              both pitched, in words
//
// Lanes are a plain loop except where a launcher reaches a kernel with a cross-lane operation (the fill plane's row pass, the
// bicubic kernels' ballot): those calls give every lane a thread.
#include "lfg_internal.hpp"
#include "on_host_frames.hpp"

using namespace on_host;

static void must(hipError_t e) { if (e != hipSuccess) die("a launcher returned an error"); }

int main(int argc, char **argv) {
    return run_manifest(argc, argv, [](const std::vector<std::string> &a) {
        const std::string &op = a[0];
        size_t i = 1;
        auto integer = [&] { return std::stoi(a.at(i++)); };
        auto real = [&] { return std::stof(a.at(i++)); };       // the test writes nine significant digits: the float itself
        auto word = [&]() -> const std::string & { return a.at(i++); };
        const int W = integer(), H = integer();
        const size_t pixels = (size_t)W * (size_t)H;
        if (op == "mc" || op == "masked" || op == "bicubic") {
            const float t = real();
            const int ms = integer(), reach = op == "bicubic" ? 0 : integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true), mv = vectors(word(), W, H, true);
            Buffer mask;
            if (op == "masked") mask = bytes(word(), W, H, true);
            Buffer out = rgba(word(), W, H, false);
            Scratch keys(pixels * 4), fill(reach ? pixels * 4 : 0);
            hip_on_host::LaneThreads threads(reach != 0 || op == "bicubic");
            const lfg_frame p = prev.frame(W, LFG_FORMAT_RGBA8_UNORM), c = curr.frame(W, LFG_FORMAT_RGBA8_UNORM), m = mv.frame(W, LFG_FORMAT_MV_S8X2),
                            o = out.frame(W, LFG_FORMAT_RGBA8_UNORM);
            uint32_t *f = reach ? (uint32_t *)fill.p : nullptr;
            if (op == "mc") must(lfg::launch_interpolate_compensated(nullptr, p, c, m, o, t, ms, (uint32_t *)keys.p, f, reach));
            else if (op == "masked") must(lfg::launch_interpolate_compensated_masked(nullptr, p, c, m, mask.mask(W), o, t, ms, (uint32_t *)keys.p, f, reach));
            else must(lfg::launch_interpolate_compensated_bicubic(nullptr, p, c, m, o, t, ms, (uint32_t *)keys.p));
            out.write();
        } else if (op == "extrapolate") {
            const float ahead = real();
            const int ms = integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true), mv = vectors(word(), W, H, true), out = rgba(word(), W, H, false);
            Scratch keys(pixels * 4);
            must(lfg::launch_extrapolate_compensated(nullptr, prev.frame(W, LFG_FORMAT_RGBA8_UNORM), curr.frame(W, LFG_FORMAT_RGBA8_UNORM),
                                                     mv.frame(W, LFG_FORMAT_MV_S8X2), out.frame(W, LFG_FORMAT_RGBA8_UNORM), ahead, ms, (uint32_t *)keys.p));
            out.write();
        } else if (op == "bidir") {
            const float t = real();
            const int ms = integer(), tolerance = integer(), reach = integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true), fwd = vectors(word(), W, H, true), bwd = vectors(word(), W, H, true);
            Buffer out = rgba(word(), W, H, false);
            Scratch keys(pixels * 4), fill(reach ? pixels * 4 : 0);
            hip_on_host::LaneThreads threads(reach != 0);
            must(lfg::launch_interpolate_compensated_bidirectional(nullptr, prev.frame(W, LFG_FORMAT_RGBA8_UNORM), curr.frame(W, LFG_FORMAT_RGBA8_UNORM),
                                                                   fwd.frame(W, LFG_FORMAT_MV_S8X2), bwd.frame(W, LFG_FORMAT_MV_S8X2),
                                                                   out.frame(W, LFG_FORMAT_RGBA8_UNORM), t, ms, tolerance, (uint32_t *)keys.p,
                                                                   reach ? (uint32_t *)fill.p : nullptr, reach));
            out.write();
        } else if (op == "consistency") {
            const int tolerance = integer();
            Buffer x = vectors(word(), W, H, true), y = vectors(word(), W, H, true), out = bytes(word(), W, H, false);
            must(lfg::launch_motion_consistency(nullptr, x.frame(W, LFG_FORMAT_MV_S8X2), y.frame(W, LFG_FORMAT_MV_S8X2), tolerance, out.mask(W)));
            out.write();
        } else if (op == "static_mask") {
            const int tolerance = integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true), out = bytes(word(), W, H, false);
            must(lfg::launch_static_mask(nullptr, prev.frame(W, LFG_FORMAT_RGBA8_UNORM), curr.frame(W, LFG_FORMAT_RGBA8_UNORM), tolerance, out.mask(W)));
            out.write();
        } else if (op == "subpel" || op == "subpel_bicubic") {
            const float t = real();
            const int ms = integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true), mvq = rgba(word(), W, H, true), out = rgba(word(), W, H, false);
            Scratch keys(pixels * 8);
            hip_on_host::LaneThreads threads(op == "subpel_bicubic");
            const lfg_frame p = prev.frame(W, LFG_FORMAT_RGBA8_UNORM), c = curr.frame(W, LFG_FORMAT_RGBA8_UNORM), m = mvq.frame(W, LFG_FORMAT_MV_S16X2_Q2),
                            o = out.frame(W, LFG_FORMAT_RGBA8_UNORM);
            if (op == "subpel") must(lfg::launch_interpolate_compensated_subpel(nullptr, p, c, m, o, t, ms, (unsigned long long *)keys.p));
            else must(lfg::launch_interpolate_compensated_subpel_bicubic(nullptr, p, c, m, o, t, ms, (unsigned long long *)keys.p));
            out.write();
        } else if (op == "fill_plane") {
            const int reach = integer(), passStatic = integer(), band = integer();
            Buffer keys = rgba(word(), W, H, true), plane = rgba(word(), W, H, false);
            hip_on_host::LaneThreads threads;
            must(lfg::launch_hole_fill_plane(nullptr, (const uint32_t *)keys.data(), keys.pitch / 4, (uint32_t *)plane.data(), plane.pitch / 4, W, H, reach,
                                             passStatic != 0, band));
            plane.write();
        } else {
            die("unknown case " + op);
        }
    });
}
