// deband.hip on the CPU through tests/cpp/hip_on_host: the file compiled by g++ as it is, and its own launch_deband run on
// frames that end where their last row ends (tests/cpp/on_host_frames.hpp) -- the 16-byte route with its remainder launch
// where lead and pitch are multiples of 16, the dword route otherwise.  The kernel has no barrier and, on the CPU, no
// cross-lane operation (the row's readfirstlane is the identity here), so its lanes are a plain loop.
// tests/test_deband_on_host.py holds every byte to tests/deband_model.py.  One case per line:
//
//   deband  W H iterations threshold radius grain seed  in out
#include "lfg_internal.hpp"
#include "on_host_frames.hpp"

using namespace on_host;

int main(int argc, char **argv) {
    return run_manifest(argc, argv, [](const std::vector<std::string> &a) {
        if (a.at(0) != "deband") die("unknown case " + a[0]);
        size_t i = 1;
        auto integer = [&] { return std::stoll(a.at(i++)); };
        const int W = (int)integer(), H = (int)integer();
        const int iterations = (int)integer(), threshold = (int)integer(), radius = (int)integer(), grain = (int)integer();
        const uint32_t seed = (uint32_t)integer();
        Buffer in = rgba(a.at(i++), W, H, true);
        Buffer out = rgba(a.at(i++), W, H, false);
        const uint32_t RGBA = LFG_FORMAT_RGBA8_UNORM;
        if (lfg::launch_deband(nullptr, in.frame(W, RGBA), out.frame(W, RGBA), iterations, threshold, radius, grain, seed) != hipSuccess)
            die("launch_deband returned an error");
        out.write();
    });
}
