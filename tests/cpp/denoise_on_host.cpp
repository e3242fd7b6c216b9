// csrc/lfg_denoise.hpp without a GPU: the header that denoise.hip takes its per-pixel arithmetic from, compiled with g++ alone.
// tests/test_denoise_on_host.py writes rows of uint32 words, this program puts each row through one function of the header and
// writes the results, and the test holds them to tests/denoise_model.py.
//   denoise_on_host weight IN OUT   rows (strength, L, cost, target inside)      -> w
//   denoise_on_host shares IN OUT   rows (L, w1, w2)                             -> a0, a1, a2
//   denoise_on_host texel  IN OUT   rows (a1, a2, limit, curr, ref1, ref2)       -> the packed texel; a0 = 256 - a1 - a2
//   denoise_on_host --limits        the ends of the parameter ranges, one line
#include <cstdio>
#include <cstring>
#include <vector>

#include "lfg_denoise.hpp"

namespace {

std::vector<uint32_t> read_words(const char *path) {
    std::vector<uint32_t> words;
    FILE *f = std::fopen(path, "rb");
    if (!f) return words;
    uint32_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, sizeof(uint32_t), 4096, f)) > 0) words.insert(words.end(), buf, buf + n);
    std::fclose(f);
    return words;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--limits")) {
        std::printf("%d %d %d %d %d\n", lfg::kDenoiseMaxRefs, lfg::kDenoiseMaxRadius, lfg::kDenoiseMaxTolerance, lfg::kDenoiseMaxStrength,
                    lfg::kDenoiseMaxLimit);
        return 0;
    }
    if (argc != 4) return 2;
    const bool weight = !std::strcmp(argv[1], "weight"), shares = !std::strcmp(argv[1], "shares"), texel = !std::strcmp(argv[1], "texel");
    const size_t cols = weight ? 4 : shares ? 3 : texel ? 6 : 0;
    if (!cols) return 2;
    const std::vector<uint32_t> in = read_words(argv[2]);
    if (in.empty() || in.size() % cols) return 3;
    std::vector<uint32_t> out;
    for (size_t i = 0; i < in.size(); i += cols) {
        const uint32_t *r = &in[i];
        if (weight) {
            out.push_back(lfg::denoise_weight(r[0], r[1], r[2], r[3] != 0u));
        } else if (shares) {
            const lfg::DenoiseShares s = lfg::denoise_shares(r[0], r[1], r[2]);
            out.insert(out.end(), s.a, s.a + 3);
        } else {
            const lfg::DenoiseShares s = {{256u - r[0] - r[1], r[0], r[1]}};
            out.push_back(lfg::denoise_texel(s, r[3], r[4], r[5], r[2]));
        }
    }
    FILE *f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size()) return 4;
    return std::fclose(f) == 0 ? 0 : 4;
}
