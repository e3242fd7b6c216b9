// Test helper (CPU only): holds csrc/lfg_record_plan.hpp -- the launch plans of the record kernels (frame_diff, frame_ssim,
// frame_histogram, pair_match) and the alignment rule of the 16-byte kernels -- to its contract, by running the cursor the
// kernels run as loops over every workgroup, every lane or wave and every trip, at CU counts (1, 2, 256) and sizes that no GPU
// test can afford.  Built with g++ alone (no ROCm include), plainly and with -fsanitize=address,undefined: a walk that leaves
// its frame is then the sanitizer's as well as a failed check.  tests/test_record_plan.py passes every constant of the kernels
// that a plan takes (K_DIFF_THREADS, K_DIFF_GROUP_PIXELS, K_PAIR_BLOCK_X ...), read from the .hip files; what a plan must keep,
// 2^31 per workgroup, is stated here.  Prints "ok <checks>" and exits 0, or prints the first failed check and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lfg_record_plan.hpp"

using namespace lfg;

namespace {

typedef unsigned long long u64;
constexpr u64 kTwo31 = 1ull << 31;                           // what a 32-bit LDS bin may count, and what the divisor is exact below

long g_checks = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        ++g_checks;                                                                                                    \
        if (!(cond)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// A seeded generator of its own: the same numbers everywhere.
u64 g_seed = 0x9E3779B97F4A7C15ull;
u64 next_random() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }

const int kCus[] = {1, 2, 256};

// What the launch functions hand to the plans as the most items of a workgroup.
constexpr u64 kDiffGroupItems = (u64)(K_DIFF_GROUP_PIXELS) / 4;                                       // an item is at most 4 pixels
constexpr u64 kSsimGroupItems = (u64)(K_SSIM_GROUP_WINDOWS) / (K_SSIM_STRIP_WINDOWS * K_SSIM_SEGMENT_ROWS);
uint32_t g_diffTripsOneCu = 0, g_ssimTripsOneCu = 0;         // the longest walks at one CU

// ---- the divisor: n / d for every n < 2^31

void check_divisor_at(uint32_t d) {
    const RecordDivisor v = record_divisor(d);
    const u64 fixed[] = {0, (u64)d - 1, d, (u64)d + 1, kTwo31 - 1};
    for (u64 n : fixed)
        if (n < kTwo31) CHECK(record_divide((uint32_t)n, v.magic, v.shift) == n / d, "d %u n %llu", d, n);
    for (int i = 0; i < 10000; ++i) {
        const uint32_t n = (uint32_t)(next_random() >> 33);                          // below 2^31
        CHECK(record_divide(n, v.magic, v.shift) == n / d, "d %u n %u", d, n);
    }
}

void check_divisor() {
    for (uint32_t d = 1; d <= 4096; ++d) check_divisor_at(d);
    for (int k = 0; k <= 31; ++k)
        for (int o = -1; o <= 1; ++o) {
            const u64 d = (1ull << k) + o;
            if (d >= 1) check_divisor_at((uint32_t)d);
        }
}

// ---- frame_diff: a lane per item, K_DIFF_UNROLL items per trip, (row, item of the row)

void check_diff_walk(uint32_t itemsX, uint32_t H, int cus) {
    RecordGrid g;
    CHECK(record_fixed_grid<u64>(itemsX, H, K_DIFF_THREADS, K_DIFF_UNROLL, K_DIFF_GROUPS_PER_CU, cus, kDiffGroupItems, g), "%u x %u refused", itemsX, H);
    if (cus == 1) g_diffTripsOneCu = std::max(g_diffTripsOneCu, g.trips);
    const RecordDivisor d = record_divisor(itemsX);
    const uint32_t stepRow = (uint32_t)(g.stride / itemsX), stepG = (uint32_t)(g.stride % itemsX);
    const u64 items = (u64)itemsX * H, pitch = (u64)itemsX * 16 + 48, itemBytes = 16;          // the byte offset rides along, as in the kernel
    std::vector<uint8_t> seen(items, 0);
    u64 visits = 0;
    for (uint32_t block = 0; block < g.grid; ++block)
        for (uint32_t tid = 0; tid < K_DIFF_THREADS; ++tid) {
            RecordCursor<u64> at = record_cursor<u64>(block * (uint32_t)K_DIFF_THREADS + tid, itemsX, d.magic, d.shift);
            u64 off = at.major * pitch + at.minor * itemBytes;
            const u64 step = stepRow * pitch + stepG * itemBytes, wrap = pitch - itemsX * itemBytes;
            for (uint32_t t = 0; t < g.trips; ++t)           // every lane the same trips: the kernel's ballots see whole waves
                for (int k = 0; k < K_DIFF_UNROLL; ++k) {
                    CHECK(at.minor < itemsX, "minor %u of %u", at.minor, itemsX);
                    if (at.major < H) {                      // an item past the end counts nowhere
                        CHECK(off == at.major * pitch + at.minor * itemBytes, "offset %llu at (%llu, %u)", off, at.major, at.minor);
                        ++seen[at.major * itemsX + at.minor];
                        ++visits;
                    }
                    off += step;
                    at.advance(stepRow, stepG, itemsX, [&] { off += wrap; });
                }
        }
    CHECK(visits == items, "%llu visits of %llu items (%u x %u, %d CUs)", visits, items, itemsX, H, cus);
    for (u64 i = 0; i < items; ++i) CHECK(seen[i] == 1, "item %llu seen %d times (%u x %u, %d CUs)", i, seen[i], itemsX, H, cus);
    CHECK((u64)g.trips * K_DIFF_THREADS * K_DIFF_UNROLL * 4 <= kTwo31, "a workgroup sees more than 2^31 pixels");
}

// ---- frame_ssim: a wave per item, (segment, strip); an item is K_SSIM_STRIP_WINDOWS x K_SSIM_SEGMENT_ROWS windows at most

void check_ssim_walk(uint32_t bw, uint32_t bh, int cus) {
    const uint32_t strips = (bw - 1u + K_SSIM_STRIP_WINDOWS - 1u) / K_SSIM_STRIP_WINDOWS;
    const uint32_t segments = (bh - 1u + K_SSIM_SEGMENT_ROWS - 1u) / K_SSIM_SEGMENT_ROWS;
    RecordGrid g;
    CHECK(record_fixed_grid<uint32_t>(strips, segments, K_SSIM_WAVES, 1, K_SSIM_GROUPS_PER_CU, cus, kSsimGroupItems, g),
          "%u x %u refused", bw, bh);
    if (cus == 1) g_ssimTripsOneCu = std::max(g_ssimTripsOneCu, g.trips);
    const RecordDivisor d = record_divisor(strips);
    const uint32_t stepSegment = (uint32_t)(g.stride / strips), stepStrip = (uint32_t)(g.stride % strips);
    const u64 items = (u64)strips * segments;
    std::vector<uint8_t> seen(items, 0);
    u64 visits = 0, windows = 0;
    for (uint32_t block = 0; block < g.grid; ++block)
        for (uint32_t wave = 0; wave < K_SSIM_WAVES; ++wave) {
            RecordCursor<uint32_t> at = record_cursor<uint32_t>(block * (uint32_t)K_SSIM_WAVES + wave, strips, d.magic, d.shift);
            for (uint32_t t = 0; t < g.trips; ++t) {
                CHECK(at.minor < strips, "minor %u of %u", at.minor, strips);
                if (at.major < segments) {
                    ++seen[(u64)at.major * strips + at.minor];
                    ++visits;
                    // the item's windows, as the kernel counts them: columns of the strip that exist, window rows of the segment
                    const u64 cols = std::min<u64>(K_SSIM_STRIP_WINDOWS, (u64)(bw - 1u) - (u64)at.minor * K_SSIM_STRIP_WINDOWS);
                    const u64 rows = std::min<u64>(K_SSIM_SEGMENT_ROWS, (u64)(bh - 1u) - (u64)at.major * K_SSIM_SEGMENT_ROWS);
                    windows += cols * rows;
                }
                at.advance(stepSegment, stepStrip, strips);
            }
        }
    CHECK(visits == items, "%llu visits of %llu items (%u x %u blocks, %d CUs)", visits, items, bw, bh, cus);
    for (u64 i = 0; i < items; ++i) CHECK(seen[i] == 1, "item %llu seen %d times (%u x %u blocks, %d CUs)", i, seen[i], bw, bh, cus);
    CHECK(windows == (u64)(bw - 1u) * (bh - 1u), "%llu windows of %llu", windows, (u64)(bw - 1u) * (bh - 1u));
    CHECK((u64)g.trips * K_SSIM_WAVES * K_SSIM_STRIP_WINDOWS * K_SSIM_SEGMENT_ROWS <= kTwo31, "a workgroup sees more than 2^31 windows");
}

// ---- the cap: whatever the plan accepts keeps a workgroup within 2^31 and every index inside its field

template <typename Major>
void check_cap_at(uint32_t minors, uint32_t majors, uint32_t walkers, uint32_t unroll, uint32_t groupsPerCu, u64 groupItems, u64 perItem,
                  int cus) {
    RecordGrid g;
    if (!record_fixed_grid<Major>(minors, majors, walkers, unroll, groupsPerCu, cus, groupItems, g)) { ++g_checks; return; }
    const u64 items = (u64)minors * majors;
    CHECK((u64)g.trips * walkers * unroll * perItem <= kTwo31, "%u x %u: a workgroup takes more than 2^31", minors, majors);
    CHECK(g.stride < kTwo31 && g.stride == (u64)g.grid * walkers, "%u x %u: stride %llu", minors, majors, g.stride);      // first < stride
    CHECK((u64)g.trips * unroll * g.stride >= items, "%u x %u: the trips do not reach the end", minors, majors);
    CHECK((u64)(g.trips - 1u) * unroll * g.stride < items, "%u x %u: a trip more than needed", minors, majors);
    // the last position a cursor takes: first + trips * unroll * stride with first = stride - 1
    const u64 last = g.stride - 1 + (u64)g.trips * unroll * g.stride;
    CHECK(last / minors <= (u64)std::numeric_limits<Major>::max(), "%u x %u: the major leaves its field", minors, majors);
    CHECK(minors <= kTwo31, "%u minors accepted", minors);
}

void check_cap() {
    for (int cus : {1, 256})
        for (int e = 0; e <= 40; ++e)
            for (int lgMinors = 0; lgMinors <= 31 && lgMinors <= e; ++lgMinors)
                for (int o = -1; o <= 1; ++o) {
                    const u64 minors = (1ull << lgMinors) + (lgMinors > 1 ? o : 0), majors = ((1ull << e) + (o > 0 ? 12345 : 0)) / minors;
                    if (majors == 0 || majors > 0xffffffffull || minors > 0xffffffffull) continue;
                    check_cap_at<u64>((uint32_t)minors, (uint32_t)majors, K_DIFF_THREADS, K_DIFF_UNROLL, K_DIFF_GROUPS_PER_CU, kDiffGroupItems, 4, cus);
                    check_cap_at<uint32_t>((uint32_t)minors, (uint32_t)majors, K_SSIM_WAVES, 1, K_SSIM_GROUPS_PER_CU, kSsimGroupItems,
                                           (u64)K_SSIM_STRIP_WINDOWS * K_SSIM_SEGMENT_ROWS, cus);
                }
    RecordGrid g;
    CHECK(!record_fixed_grid<u64>(0x80000001u, 1, K_DIFF_THREADS, K_DIFF_UNROLL, K_DIFF_GROUPS_PER_CU, 256, kDiffGroupItems, g), "2^31 + 1 minors accepted");
    CHECK(!record_fixed_grid<uint32_t>(1, 0xffffffffu, K_SSIM_WAVES, 1, K_SSIM_GROUPS_PER_CU, 256, kSsimGroupItems, g), "a major beyond 32 bits accepted");
    CHECK(record_fixed_grid<u64>(1, 0xffffffffu, K_DIFF_THREADS, K_DIFF_UNROLL, K_DIFF_GROUPS_PER_CU, 256, kDiffGroupItems, g), "a 64-bit major refused");
}

// ---- frame_histogram: the row's items and the workgroup's rectangle

void check_hist_at(uint32_t W, uint32_t lead, size_t pitch) {
    const uintptr_t base = 0x10000u + lead;
    const HistRow r = hist_row((const void *)base, pitch, W);
    CHECK(r.head + 4u * r.wideItems + r.tail == W && r.itemsX == r.wideItems + r.head + r.tail, "W %u lead %u pitch %zu", W, lead, pitch);
    std::vector<uint8_t> pixel(W, 0);
    for (uint32_t g = 0; g < r.itemsX; ++g) {
        const bool wide = g < r.wideItems;
        const uint32_t x = hist_item_x(r, g, wide), n = wide ? 4u : 1u;
        CHECK(x + n <= W, "item %u at %u of %u", g, x, W);
        for (uint32_t i = 0; i < n; ++i) ++pixel[x + i];
        if (wide)
            for (uint32_t y = 0; y < 3; ++y) CHECK((base + y * pitch + (size_t)x * 4u) % 16u == 0, "W %u lead %u pitch %zu item %u row %u", W, lead, pitch, g, y);
    }
    for (uint32_t x = 0; x < W; ++x) CHECK(pixel[x] == 1, "pixel %u in %d items (W %u lead %u pitch %zu)", x, pixel[x], W, lead, pitch);

    // the rectangle, as the kernel walks it: along the row by gridDim.x * bx, down the frame by gridDim.y * by * unroll
    for (uint32_t H : {1u, 37u, 131u})
        for (int cus : {1, 256}) {
            HistGrid g;
            CHECK(hist_grid(r.itemsX, H, K_HIST_THREADS, K_HIST_UNROLL, K_HIST_GROUPS_PER_CU, cus, K_HIST_GROUP_PIXELS, g), "W %u H %u refused", W, H);
            const uint32_t bx = 1u << g.lgBx, by = (uint32_t)K_HIST_THREADS >> g.lgBx;
            CHECK(g.lgBx >= 6 && g.lgBx <= 10 && g.groupsX >= 1 && g.groupsY >= 1 && g.groupsY <= 65535u, "lgBx %u grid %u x %u", g.lgBx, g.groupsX, g.groupsY);
            std::vector<uint8_t> seen((size_t)r.itemsX * H, 0);
            u64 most = 0;
            for (uint32_t gy = 0; gy < g.groupsY; ++gy)
                for (uint32_t gx = 0; gx < g.groupsX; ++gx) {
                    u64 trips = 0;
                    for (u64 g0 = (u64)gx * bx; g0 < r.itemsX; g0 += (u64)g.groupsX * bx)
                        for (u64 y0 = (u64)gy * by * K_HIST_UNROLL; y0 < H; y0 += (u64)g.groupsY * by * K_HIST_UNROLL) {
                            ++trips;                         // of every lane of the workgroup: the bounds hold no lane index
                            for (uint32_t tid = 0; tid < K_HIST_THREADS; ++tid)
                                for (int k = 0; k < K_HIST_UNROLL; ++k) {
                                    const u64 item = g0 + (tid & (bx - 1u)), y = y0 + (u64)k * by + (tid >> g.lgBx);
                                    if (item < r.itemsX && y < H) ++seen[(size_t)(y * r.itemsX + item)];
                                }
                        }
                    most = std::max(most, trips);
                }
            for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "item %zu seen %d times (W %u H %u, %d CUs)", i, seen[i], W, H, cus);
            CHECK(most * K_HIST_THREADS * K_HIST_UNROLL * 4 <= kTwo31, "a workgroup sees more than 2^31 pixels");
        }
}

void check_hist() {
    std::vector<uint32_t> widths;
    for (uint32_t w = 1; w <= 70; ++w) widths.push_back(w);
    for (uint32_t w : {255u, 256u, 257u, 258u, 1023u, 1024u, 1025u, 1026u}) widths.push_back(w);
    for (uint32_t W : widths)
        for (uint32_t lead : {0u, 4u, 8u, 12u})
            for (size_t slack : {(size_t)0, (size_t)4, (size_t)8, (size_t)16}) {
                const size_t pitch = ((size_t)W * 4u + 15u) / 16u * 16u + slack;      // multiples of 16 and not
                check_hist_at(W, lead, pitch);
            }
    // a frame beyond any device: the trips bound refuses instead of letting a bin wrap
    HistGrid g;
    CHECK(!hist_grid(0x20000000u, 0xffffffffu, K_HIST_THREADS, K_HIST_UNROLL, K_HIST_GROUPS_PER_CU, 1, K_HIST_GROUP_PIXELS, g), "2^61 pixels on one CU accepted");
}

// ---- pair_match: every tile once, two per trip

void check_pair() {
    const uint32_t sizes[][2] = {{1, 1}, {64, 4}, {65, 5}, {257, 131}, {1920, 1080}, {3, 9000}};
    const uint32_t bx = K_PAIR_BLOCK_X, by = K_PAIR_BLOCK_Y, unroll = K_PAIR_UNROLL;
    for (auto &s : sizes)
        for (int cus : kCus) {
            const PairGrid g = pair_grid(s[0], s[1], bx, by, unroll, K_PAIR_GROUPS_PER_CU, cus);
            CHECK(g.tilesX == (s[0] + bx - 1u) / bx && g.tiles == g.tilesX * ((s[1] + by - 1u) / by) && g.grid >= 1u &&
                  g.grid <= (uint32_t)K_PAIR_GROUPS_PER_CU * (uint32_t)cus, "%u x %u", s[0], s[1]);
            std::vector<uint8_t> seen(g.tiles, 0);
            for (uint32_t block = 0; block < g.grid; ++block)
                for (uint32_t t0 = block; t0 < g.tiles; t0 += g.grid * unroll)
                    for (uint32_t k = 0; k < unroll; ++k)
                        if (t0 + k * g.grid < g.tiles) ++seen[t0 + k * g.grid];
            for (uint32_t t = 0; t < g.tiles; ++t) CHECK(seen[t] == 1, "tile %u seen %d times (%u x %u, %d CUs)", t, seen[t], s[0], s[1], cus);
        }
}

// ---- the alignment rule and the split of a width

void check_split() {
    const uintptr_t off[] = {0, 4, 8, 12, 16, 20};
    for (uint32_t W = 0; W <= 70; ++W)
        for (uintptr_t a : off)
            for (uintptr_t b : off)
                for (uintptr_t pa : off)
                    for (uintptr_t pb : off) {
                        const bool every = a % 16 == 0 && b % 16 == 0 && pa % 16 == 0 && pb % 16 == 0;
                        const bool aligned = multiples_of_16((const void *)(0x4000 + a), (void *)(0x8000 + b), (size_t)(256 + pa), (uint32_t)(512 + pb));
                        CHECK(aligned == every, "offsets %zu %zu %zu %zu", (size_t)a, (size_t)b, (size_t)pa, (size_t)pb);
                        const uint32_t wideW = wide_columns(aligned, W), rest = W - wideW;
                        CHECK(wideW % 4u == 0 && wideW + rest == W && rest <= W, "W %u", W);
                        CHECK(every ? wideW == (W & ~3u) && rest < 4u : wideW == 0u, "W %u: %u wide", W, wideW);
                    }
}

}  // namespace

int main() {
    check_divisor();
    const uint32_t diffSizes[][2] = {{1, 1}, {7, 5}, {1025, 3}, {257, 131}, {1500, 40}, {3, 9000}};       // itemsX x H
    const uint32_t ssimSizes[][2] = {{2, 2}, {65, 10}, {200, 300}, {480, 270}, {64, 4000}};              // blocks bw x bh
    for (int cus : kCus) {
        for (auto &s : diffSizes) check_diff_walk(s[0], s[1], cus);
        for (auto &s : ssimSizes) check_ssim_walk(s[0], s[1], cus);
    }
    // the walks above are the multi-trip ones the check exists for: with today's constants 257 x 131 items of frame_diff are 9
    // trips of a lane at one CU and 1500 x 40 are 15, 64 x 4000 blocks of frame_ssim 32 trips of a wave
    CHECK(g_diffTripsOneCu >= 9u && g_ssimTripsOneCu >= 32u, "the longest walks at one CU: %u and %u trips", g_diffTripsOneCu, g_ssimTripsOneCu);
    check_cap();
    check_hist();
    check_pair();
    check_split();
    std::printf("ok %ld checks\n", g_checks);
    return 0;
}
