// csrc/lfg_levels.hpp on the CPU, with g++ alone (tests/test_levels_on_host.py): the map rule and both apply bodies, as the
// kernels of csrc/levels.hip run them.  Built plainly and with -fsanitize=address,undefined; every buffer is an allocation of
// exactly the size it should have, so a table index or a record word out of range is a reported read or write.
//
//   levels_on_host match FROM.bin TO.bin MIN_SHIFT16 MAP.bin        two records of 1,025 words -> the 1,560 bytes of a map
//   levels_on_host apply W H IN.bin MAP.bin MODE FACTOR OUT.bin      W * H texels through the map (MODE 0: forward, 1: at FACTOR)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lfg_levels.hpp"

namespace {

template <typename T>
bool read_all(const char *path, std::vector<T> &data, size_t count) {
    data.resize(count);
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    const size_t got = fread(data.data(), sizeof(T), count, f);
    const bool end = fgetc(f) == EOF;
    fclose(f);
    if (got != count || !end) { fprintf(stderr, "%s does not hold exactly %zu items\n", path, count); return false; }
    return true;
}

template <typename T>
bool write_all(const char *path, const std::vector<T> &data) {
    FILE *f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    const bool ok = fwrite(data.data(), sizeof(T), data.size(), f) == data.size();
    return fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "match" && argc == 6) {
        std::vector<uint64_t> from, to;
        if (!read_all(argv[2], from, lfg::kHistWords) || !read_all(argv[3], to, lfg::kHistWords)) return 1;
        std::vector<uint8_t> map(lfg::kMapBytes);
        lfg::levels_match_host(from.data(), to.data(), atoi(argv[4]), map.data());
        return write_all(argv[5], map) ? 0 : 1;
    }
    if (mode == "apply" && argc == 9) {
        const size_t pixels = (size_t)atoi(argv[2]) * (size_t)atoi(argv[3]);
        std::vector<uint32_t> in, out(pixels);
        std::vector<uint8_t> map;
        if (!read_all(argv[4], in, pixels) || !read_all(argv[5], map, lfg::kMapBytes)) return 1;
        const uint8_t *forward = map.data() + lfg::kMapHeadBytes, *inverse = forward + lfg::kLevelChannels * lfg::kLevels;
        // the table as the kernel stages it: forward, or inverse combined with the identity at tq
        std::vector<uint8_t> table((size_t)lfg::kLevelChannels * lfg::kLevels);
        const int at = atoi(argv[6]), tq = at ? lfg::levels_tq(strtof(argv[7], nullptr)) : 0;
        for (size_t i = 0; i < table.size(); ++i) table[i] = at ? (uint8_t)lfg::levels_at(inverse[i], (uint32_t)(i & 255u), tq) : forward[i];
        for (size_t i = 0; i < pixels; ++i) out[i] = lfg::levels_texel(table.data(), in[i]);
        return write_all(argv[8], out) ? 0 : 1;
    }
    fprintf(stderr, "usage: levels_on_host match FROM TO MIN_SHIFT16 MAP | apply W H IN MAP MODE FACTOR OUT\n");
    return 2;
}
