// The launch plans of the kernels that reduce a frame to a small device record (pair_stats.hip, frame_diff.hip, frame_ssim.hip,
// levels.hip), and what the kernels that move 16 bytes at a time ask of their frames (those, sharpen.hip, static_mask.hip): all
// the arithmetic that decides which lane visits which item, as plain functions of the sizes and the device's CU count.  Host
// and device code share this header; it needs nothing but the standard library, so that the kernels and
// tests/cpp/record_plan_check.cpp, built with g++ alone, run the same text -- the check runs every plan as loops over every lane
// and every trip, with CU counts and sizes that no GPU test can afford.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define LFG_RECORD_FN __host__ __device__ __forceinline__
#else
#define LFG_RECORD_FN inline
#endif

namespace lfg {

// ---- 16 bytes at a time

// Every base and pitch given is a multiple of 16: what lets a kernel take four pixels of a row through one 16-byte access.
template <typename... T>
inline bool multiples_of_16(T... baseOrPitch) { return (((uintptr_t)baseOrPitch | ...) % 16u) == 0; }

// The columns of a row of W pixels that go four at a time where `aligned` (the frames' multiples_of_16): those up to the last
// multiple of 4.  An item is never partial: the 0 .. 3 columns that remain -- all W where nothing is aligned -- go one by one.
inline uint32_t wide_columns(bool aligned, uint32_t W) { return aligned ? W & ~3u : 0u; }

// ---- division by a multiplier

// n / d for every n < 2^31 as (n * magic) >> shift, for any d >= 1: with 2^(l-1) < d <= 2^l, magic = ceil(2^(31+l) / d)
// <= 2^32 and shift = 31 + l <= 63 (Granlund and Montgomery 1994, theorem 4.2); n * magic < 2^63.  What the kernels divide
// with instead of the compiler's division, which goes through a float reciprocal.
struct RecordDivisor { unsigned long long magic; uint32_t shift; };

inline RecordDivisor record_divisor(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < (unsigned long long)d) ++l;
    const uint32_t shift = 31u + l;
    return RecordDivisor{((1ull << shift) + d - 1ull) / d, shift};
}

LFG_RECORD_FN unsigned long long record_divide(uint32_t n, unsigned long long magic, uint32_t shift) {
    return ((unsigned long long)n * magic) >> shift;
}

// ---- the walk of a fixed grid

// The items of a launch are numbered major * minors + minor (frame_diff: row and item of the row; frame_ssim: segment and
// strip).  A walker -- a lane or a wave -- starts at item `first` and goes on in steps of the launch's stride, which the host
// hands over as (stride / minors, stride % minors): no division on the way.  Major is the kernel's type for the major index.
template <typename Major>
struct RecordCursor {
    Major major;
    uint32_t minor;

    // One step on.  onWrap() runs where the minor wrapped, for what rides along (frame_diff's two byte offsets): inside the one
    // branch -- a flag handed back instead costs frame_diff_kernel 30 instructions of selects per item.
    template <typename OnWrap>
    LFG_RECORD_FN void advance(uint32_t stepMajor, uint32_t stepMinor, uint32_t minors, OnWrap onWrap) {
        minor += stepMinor;
        major += stepMajor;
        if (minor >= minors) { minor -= minors; ++major; onWrap(); }
    }
    LFG_RECORD_FN void advance(uint32_t stepMajor, uint32_t stepMinor, uint32_t minors) {
        advance(stepMajor, stepMinor, minors, [] {});
    }
};

// The cursor on item `first` < 2^31, by value; (magic, shift) is record_divisor(minors).
template <typename Major>
LFG_RECORD_FN RecordCursor<Major> record_cursor(uint32_t first, uint32_t minors, unsigned long long magic, uint32_t shift) {
    RecordCursor<Major> at;
    at.major = (Major)record_divide(first, magic, shift);
    at.minor = first - (uint32_t)at.major * minors;
    return at;
}

// The fixed grid: groupsPerCu workgroups per CU, never more than there is work, never so few that one workgroup would take
// more than groupItemsMost items -- what keeps its 32-bit LDS bins exact.  A workgroup has `walkers` of them, a trip is
// `unroll` items per walker, and every walker runs the same `trips`; the cursor's steps are (stride / minors, stride % minors).
struct RecordGrid { uint32_t grid, trips; unsigned long long stride; };

// False is the refusal, and one rule serves every kernel: each value a cursor takes must fit its field.
//   * first < stride < 2^31 and minors <= 2^31: record_divide is exact, and minor + stepMinor < 2 * minors fits 32 bits;
//   * a cursor ends on item first + trips * unroll * stride < items + (unroll + 1) * stride, whose major must fit Major (the
//     kernels compare it with `majors` after the last step as before it);
//   * trips fits the kernels' 32-bit argument.
// No frame a device holds comes near any of them.  A workgroup takes trips * walkers * unroll <= items / grid + walkers * unroll
// items (trips, rounded up), which `atLeast` keeps within groupItemsMost.
template <typename Major>
inline bool record_fixed_grid(uint32_t minors, uint32_t majors, uint32_t walkers, uint32_t unroll, uint32_t groupsPerCu, int deviceCus,
                              unsigned long long groupItemsMost, RecordGrid &out) {
    const unsigned long long items = (unsigned long long)minors * majors, perTrip = (unsigned long long)walkers * unroll;
    if (minors == 0u || minors > 0x80000000u || groupItemsMost <= perTrip) return false;
    const unsigned long long atLeast = items / (groupItemsMost - perTrip) + 1ull;
    const unsigned long long fixed = (unsigned long long)std::max(deviceCus, 1) * groupsPerCu;
    const unsigned long long grid = std::max(std::min((items + perTrip - 1) / perTrip, fixed), atLeast);
    const unsigned long long stride = grid * walkers;
    if (stride >= 0x80000000ull) return false;
    const unsigned long long trips = (items + stride * unroll - 1) / (stride * unroll);
    const unsigned long long lastMajor = (items + (unroll + 1ull) * stride) / minors;
    if (trips > 0xffffffffull || lastMajor > (unsigned long long)std::numeric_limits<Major>::max()) return false;
    out = RecordGrid{(uint32_t)grid, (uint32_t)trips, stride};
    return true;
}

// ---- pair_match: 64 x 4 tiles, workgroup g takes tiles g, g + grid, ..., two per trip

struct PairGrid { uint32_t tilesX, tiles, grid; };

inline PairGrid pair_grid(uint32_t W, uint32_t H, uint32_t tileW, uint32_t tileH, uint32_t unroll, uint32_t groupsPerCu, int deviceCus) {
    const uint32_t tilesX = (W + tileW - 1u) / tileW, tiles = tilesX * ((H + tileH - 1u) / tileH);
    const uint32_t trips = (tiles + unroll - 1u) / unroll;
    return PairGrid{tilesX, tiles, std::min<uint32_t>(trips, (uint32_t)std::max(deviceCus, 1) * groupsPerCu)};
}

// ---- frame_histogram: a row's items, and the workgroup's rectangle of lanes

// Item g of a row: the 16-byte items first, then the pixels in front of them and behind them.
struct HistRow {
    uint32_t W, itemsX, wideItems, head, tail;              // head + 4 * wideItems + tail = W
};

// The first pixel of item g < itemsX of a row; the item is four pixels where it is `wide`, g < wideItems, and one otherwise
// (the caller has asked, so it passes the answer).
LFG_RECORD_FN uint32_t hist_item_x(const HistRow &r, uint32_t g, bool wide) {
    const uint32_t e = g - r.wideItems;                      // pixel e of the head and the tail
    return wide ? r.head + 4u * g : (e < r.head ? e : r.W - r.tail + (e - r.head));
}

inline HistRow hist_row(const void *base, size_t pitch, uint32_t W) {
    HistRow r{};
    r.W = W;
    if (multiples_of_16(pitch)) {                            // every row meets its first 16-byte boundary after the same pixels
        r.head = std::min<uint32_t>((uint32_t)((0u - (uintptr_t)base) & 15u) / 4u, W);
        r.wideItems = (W - r.head) / 4u;
        r.tail = W - r.head - 4u * r.wideItems;
    } else {
        r.head = W;
    }
    r.itemsX = r.wideItems + r.head + r.tail;
    return r;
}

// The workgroup is 2^lgBx lanes wide and threads >> lgBx high, the grid groupsX x groupsY of them; a lane takes `unroll` rows
// per trip down the frame.
struct HistGrid { uint32_t lgBx, groupsX, groupsY; };

// False: a workgroup would see more than groupPixelsMost pixels (no frame a device holds comes near).
inline bool hist_grid(uint32_t itemsX, uint32_t H, uint32_t threads, uint32_t unroll, uint32_t groupsPerCu, int deviceCus,
                      unsigned long long groupPixelsMost, HistGrid &out) {
    // the workgroup's rectangle: the power of two bx in [64, 1024] whose multiples cover itemsX with the fewest idle lanes
    uint32_t lgBx = 6;
    unsigned long long best = ~0ull;
    for (uint32_t lg = 6; lg <= 10; ++lg) {
        const unsigned long long bx = 1ull << lg, cover = ((unsigned long long)itemsX + bx - 1) / bx * bx;
        if (cover <= best) { best = cover; lgBx = lg; }       // ties: the wider one, whose workgroup reads longer runs
    }
    const unsigned long long bx = 1ull << lgBx, by = (unsigned long long)threads >> lgBx;
    const unsigned long long fixed = (unsigned long long)std::max(deviceCus, 1) * groupsPerCu;
    const unsigned long long groupsX = std::min(((unsigned long long)itemsX + bx - 1) / bx, fixed);
    const unsigned long long rowTrips = ((unsigned long long)H + by * unroll - 1) / (by * unroll);
    const unsigned long long groupsY = std::min(std::max(fixed / groupsX, 1ull), std::min(rowTrips, 65535ull));
    // a workgroup sees at most its trips along the row times its trips down the frame times its lanes, of at most 4 pixels each
    const unsigned long long tripsX = ((unsigned long long)itemsX + groupsX * bx - 1) / (groupsX * bx);
    const unsigned long long tripsY = (rowTrips + groupsY - 1) / groupsY;
    if (tripsX * tripsY > groupPixelsMost / (4ull * threads * unroll)) return false;
    out = HistGrid{lgBx, (uint32_t)groupsX, (uint32_t)groupsY};
    return true;
}

}  // namespace lfg
