// csrc/lfg_bicubic.hpp on the CPU, with g++ alone (tests/test_bicubic_on_host.py builds this twice, plainly and with
// -fsanitize=address,undefined, and holds what it writes to tests/bicubic_model.py bit for bit).
//
//   bicubic_on_host fetch W H image.bin positions.bin out.bin
//       image.bin: W * H RGBA8 texels, tight; positions.bin: N pairs of floats (px, py); out.bin: N x 4 floats, the sample values.
//       The 16 texel words of a fetch are gathered as the kernels' taps gather them (lfg_interp.hpp: bicubic_taps, bicubic_load)
//       from an allocation of exactly W * H words, so a footprint that left its clamp would be a read out of bounds.
//   bicubic_on_host convert
//       bicubic_p_to_float against ((float)p / 255.0f) * 2^-8 for every p in [0, 65280]; prints the number of mismatches.
//   bicubic_on_host table out.bin
//       bicubic_row for phi = 0 .. 64 as 65 x 4 int32.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lfg_bicubic.hpp"

namespace {

template <typename T>
std::vector<T> read_all(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
    std::fclose(f);
    return v;
}

template <typename T>
void write_all(const char *path, const std::vector<T> &v) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
    std::fclose(f);
}

int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "convert")) {
        long bad = 0;
        for (int p = 0; p <= lfg::kBicubicPMax; ++p) {
            const float want = ((float)p / 255.0f) * 0.00390625f, got = lfg::bicubic_p_to_float(p);
            bad += std::memcmp(&want, &got, sizeof want) != 0;
        }
        std::printf("%ld\n", bad);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "table")) {
        std::vector<int32_t> rows;
        for (int phi = 0; phi <= 64; ++phi)
            for (int k = 0; k < 4; ++k) rows.push_back(lfg::bicubic_row(phi).w[k]);
        write_all(argv[2], rows);
        return 0;
    }
    if (argc != 7 || std::strcmp(argv[1], "fetch")) {
        std::fprintf(stderr, "usage: bicubic_on_host fetch W H image positions out | convert | table out\n");
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
    const std::vector<uint32_t> img = read_all<uint32_t>(argv[4]);
    const std::vector<float> pos = read_all<float>(argv[5]);
    if (W <= 0 || H <= 0 || img.size() != (size_t)W * (size_t)H || pos.size() % 2) { std::fprintf(stderr, "bad sizes\n"); return 2; }
    std::vector<float> out;
    for (size_t n = 0; n < pos.size(); n += 2) {
        const float u = pos[n] - 0.5f, v = pos[n + 1] - 0.5f;
        const float fu = std::floor(u), fv = std::floor(v);
        const int i0 = (int)fu, j0 = (int)fv;
        uint32_t t[16];
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k)
                t[4 * r + k] = img[(size_t)clampi(j0 - 1 + r, 0, H - 1) * (size_t)W + (size_t)clampi(i0 - 1 + k, 0, W - 1)];
        const lfg::BicubicP p = lfg::bicubic_p(t, lfg::bicubic_phase(u - fu), lfg::bicubic_phase(v - fv));
        for (int c = 0; c < 4; ++c) out.push_back(lfg::bicubic_p_to_float(p.p[c]));
    }
    write_all(argv[6], out);
    return 0;
}
