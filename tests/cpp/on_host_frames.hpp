// What the drivers of tests/cpp/*_on_host.cpp over tests/cpp/hip_on_host share: buffers that end where their last row ends,
// and the manifest of cases that tests/on_host_kit.py writes.
//
// A buffer is named "path:lead:pitch:poison" and is its own malloc of exactly lead + (H - 1) * pitch + W * bpp bytes, filled
// with 0x5A; an input's rows come from `path` (tight rows).  poison = 1: the lead bytes and every row's padding are poisoned
// for ASan (a no-op in a build without it): the caller passes lead and pitch as multiples of 8, so the 8-byte granules express
// the padding exactly.  An output is written to `path` whole, lead and padding included, so the caller can see that nothing but
// the rows was written.  A build with -fsanitize=address sees every byte read or written outside such a buffer.
#pragma once
#include <sanitizer/asan_interface.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "linuxfg_hip.h"

namespace on_host {

[[noreturn]] inline void die(const std::string &what) {
    fprintf(stderr, "on_host driver: %s\n", what.c_str());
    exit(2);
}

struct Buffer {
    std::string path;
    uint8_t *base = nullptr;
    size_t lead = 0, pitch = 0, widthBytes = 0, size = 0;
    int H = 0;
    bool poison = false;

    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept { *this = std::move(o); }
    Buffer &operator=(Buffer &&o) noexcept {
        release();
        path = o.path; base = o.base; lead = o.lead; pitch = o.pitch; widthBytes = o.widthBytes; size = o.size; H = o.H; poison = o.poison;
        o.base = nullptr;
        return *this;
    }
    ~Buffer() { release(); }
    uint8_t *data() const { return base + lead; }

    // spec "path:lead:pitch:poison"; rows of widthBytes; input: the rows are read from the file
    Buffer(const std::string &spec, size_t widthBytes_, int H_, bool input) {
        std::vector<std::string> part;
        std::stringstream in(spec);
        for (std::string p; std::getline(in, p, ':');) part.push_back(p);
        if (part.size() != 4) die("a buffer is path:lead:pitch:poison, not " + spec);
        path = part[0]; lead = std::stoul(part[1]); pitch = std::stoul(part[2]); poison = part[3] == "1";
        widthBytes = widthBytes_; H = H_;
        if (H < 1 || pitch < widthBytes) die("a buffer of no rows or a pitch below its width: " + spec);
        size = lead + (size_t)(H - 1) * pitch + widthBytes;
        base = (uint8_t *)malloc(size);
        if (!base || (uintptr_t)base % 16) die("malloc gave nothing or less than 16-byte alignment");
        memset(base, 0x5A, size);
        if (input) {
            FILE *f = fopen(path.c_str(), "rb");
            if (!f) die("cannot read " + path);
            for (int y = 0; y < H; ++y)
                if (fread(data() + (size_t)y * pitch, 1, widthBytes, f) != widthBytes) die("short file " + path);
            fclose(f);
        }
        set_poison(true);
    }
    void set_poison(bool on) {
        if (!poison || !base) return;
        if (lead % 8 || pitch % 8) die("a poisoned buffer has lead and pitch in multiples of 8");
        if (on) ASAN_POISON_MEMORY_REGION(base, lead); else ASAN_UNPOISON_MEMORY_REGION(base, lead);
        for (int y = 0; y + 1 < H; ++y) {
            uint8_t *pad = data() + (size_t)y * pitch + widthBytes;
            if (on) ASAN_POISON_MEMORY_REGION(pad, pitch - widthBytes); else ASAN_UNPOISON_MEMORY_REGION(pad, pitch - widthBytes);
        }
    }
    void write() {
        set_poison(false);
        FILE *f = fopen(path.c_str(), "wb");
        if (!f || fwrite(base, 1, size, f) != size) die("cannot write " + path);
        fclose(f);
        set_poison(true);
    }
    void release() {
        if (!base) return;
        set_poison(false);
        free(base);
        base = nullptr;
    }
    lfg_frame frame(int W, uint32_t format) const {
        lfg_frame f{};
        f.data = data(); f.width = (uint32_t)W; f.height = (uint32_t)H; f.pitch = (uint32_t)pitch; f.format = format;
        return f;
    }
    lfg_mask mask(int W) const { return lfg_mask{data(), (uint32_t)W, (uint32_t)H, (uint32_t)pitch}; }
};

inline Buffer rgba(const std::string &spec, int W, int H, bool input) { return Buffer(spec, (size_t)W * 4, H, input); }
inline Buffer vectors(const std::string &spec, int W, int H, bool input) { return Buffer(spec, (size_t)W * 2, H, input); }
inline Buffer bytes(const std::string &spec, int W, int H, bool input) { return Buffer(spec, (size_t)W, H, input); }

// A scratch area of exactly `bytes` bytes that the kernels own (a key image, a fill plane, a record): its own malloc, 0x5A.
struct Scratch {
    uint8_t *p;
    explicit Scratch(size_t bytes) : p((uint8_t *)malloc(bytes ? bytes : 1)) { if (!p) die("malloc"); memset(p, 0x5A, bytes); }
    Scratch(const Scratch &) = delete;
    ~Scratch() { free(p); }
};

// The manifest: one case per line, words separated by blanks.  run_manifest calls `one(words)` per line and prints "ok <n>".
template <typename F>
inline int run_manifest(int argc, char **argv, F one) {
    if (argc != 2) die("one argument: the manifest of cases");
    FILE *f = fopen(argv[1], "r");
    if (!f) die(std::string("cannot read ") + argv[1]);
    std::string text;
    char chunk[4096];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) text.append(chunk, n);
    fclose(f);
    std::stringstream lines(text);
    int cases = 0;
    for (std::string line; std::getline(lines, line);) {
        std::vector<std::string> words;
        std::stringstream in(line);
        for (std::string w; in >> w;) words.push_back(w);
        if (words.empty()) continue;
        one(words);
        ++cases;
    }
    printf("ok %d\n", cases);
    return 0;
}

}  // namespace on_host
