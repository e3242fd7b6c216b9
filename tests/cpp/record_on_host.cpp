// The record kernels on the CPU through tests/cpp/hip_on_host: pair_stats.hip, frame_diff.hip, frame_ssim.hip and levels.hip
// compiled by g++ as they are (over lfg_record.hpp's wave sums, ballots and readlane), and their own launch_* functions run on
// frames that end where their last row ends (tests/cpp/on_host_frames.hpp).  A record or a map is its own allocation of exactly
// its size.  tests/test_record_on_host.py holds every record, map and frame to the stage's CPU model.  One case per line:
//
//   pair   W H matchSad cus        prev curr mv stats                  stats: 24 bytes
//   cut    W H permille cus count  stats prev curr out.. factor..      stats: 24 bytes, read
//   diff   W H mask cus repeat     a b stats                           2,088 bytes; repeat 2: a second call that accumulates
//   ssim   W H mask cus repeat     a b stats                           568 bytes
//   hist   W H cus repeat          frame stats                         8,200 bytes
//   match  1 1 minShift16          from to map                         8,200 bytes each, read; map: 1,560 bytes
//   apply  W H mode tq             in map out
//
// Every launch gives its lanes threads where the kernel has a barrier or a cross-lane operation (the layer learns which do).
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
        const uint32_t RGBA = LFG_FORMAT_RGBA8_UNORM;
        hip_on_host::LaneThreads threads;
        if (op == "pair") {
            const int ms = integer(), cus = integer();
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true), mv = vectors(word(), W, H, true);
            Buffer stats(word(), sizeof(lfg_pair_stats), 1, false);
            must(lfg::launch_pair_match(nullptr, prev.frame(W, RGBA), curr.frame(W, RGBA), mv.frame(W, LFG_FORMAT_MV_S8X2), ms, cus, stats.data()));
            stats.write();
        } else if (op == "cut") {
            const int permille = integer(), cus = integer(), count = integer();
            Buffer stats(word(), sizeof(lfg_pair_stats), 1, true);
            Buffer prev = rgba(word(), W, H, true), curr = rgba(word(), W, H, true);
            std::vector<Buffer> outs;
            std::vector<lfg_frame> frames;
            std::vector<const lfg_frame *> pointers;
            std::vector<float> factors;
            for (int k = 0; k < count; ++k) outs.push_back(rgba(word(), W, H, false));
            for (int k = 0; k < count; ++k) { frames.push_back(outs[k].frame(W, RGBA)); factors.push_back(std::stof(word())); }
            for (int k = 0; k < count; ++k) pointers.push_back(&frames[k]);
            must(lfg::launch_cut_fallback(nullptr, prev.frame(W, RGBA), curr.frame(W, RGBA), stats.data(), permille, pointers.data(), factors.data(), count, cus));
            for (Buffer &o : outs) o.write();
        } else if (op == "diff" || op == "ssim") {
            const int mask = integer(), cus = integer(), repeat = integer();
            Buffer x = rgba(word(), W, H, true), y = rgba(word(), W, H, true);
            Buffer stats(word(), op == "diff" ? sizeof(lfg_frame_diff_stats) : sizeof(lfg_frame_ssim_stats), 1, false);
            for (int r = 0; r < repeat; ++r) {
                if (op == "diff") must(lfg::launch_frame_diff(nullptr, x.frame(W, RGBA), y.frame(W, RGBA), (uint32_t)mask, r > 0, cus, stats.data()));
                else must(lfg::launch_frame_ssim(nullptr, x.frame(W, RGBA), y.frame(W, RGBA), (uint32_t)mask, r > 0, cus, stats.data()));
            }
            stats.write();
        } else if (op == "hist") {
            const int cus = integer(), repeat = integer();
            Buffer frame = rgba(word(), W, H, true);
            Buffer stats(word(), sizeof(lfg_frame_histogram_stats), 1, false);
            for (int r = 0; r < repeat; ++r) must(lfg::launch_frame_histogram(nullptr, frame.frame(W, RGBA), r > 0, cus, stats.data()));
            stats.write();
        } else if (op == "match") {
            const int minShift16 = integer();
            Buffer from(word(), sizeof(lfg_frame_histogram_stats), 1, true), to(word(), sizeof(lfg_frame_histogram_stats), 1, true);
            Buffer map(word(), sizeof(lfg_levels_map), 1, false);
            must(lfg::launch_levels_match(nullptr, from.data(), to.data(), minShift16, map.data()));
            map.write();
        } else if (op == "apply") {
            const int mode = integer(), tq = integer();
            Buffer in = rgba(word(), W, H, true);
            Buffer map(word(), sizeof(lfg_levels_map), 1, true);
            Buffer out = rgba(word(), W, H, false);
            must(lfg::launch_levels_apply(nullptr, in.frame(W, RGBA), out.frame(W, RGBA), map.data(), mode, tq));
            out.write();
        } else {
            die("unknown case " + op);
        }
    });
}
