// Test helper (CPU only): holds csrc/lfg_table_cache.hpp -- the upload, the bounded table cache and the grow-only lane buffer
// of the C-ABI layer -- to its contract on a fake device that counts.  Built with g++ alone (no ROCm include), plainly and with
// -fsanitize=address,undefined: a block is a malloc of exactly its size, so a double free or a use of a freed table is the
// sanitizer's as well as the fake's.  Prints "ok <checks>" and exits 0, or prints the first failed check and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "lfg_table_cache.hpp"

namespace {

// The fake device: blocks are host mallocs; counts every call, keeps the outstanding blocks and the order of events, fails the
// n-th allocation or copy from now on request, and aborts on a free of what is not outstanding.
struct Fake {
    static inline int allocations = 0, frees = 0, copies = 0, fail_allocation_in = 0, fail_copy_in = 0;
    static inline std::set<void *> outstanding;
    static inline std::string log;                       // 'S' before_free / synchronize, 'A' allocate, 'F' free, 'C' copy
    static inline std::vector<void *> freed;             // in order
    static constexpr int kNoMemory = 2, kCopyFailed = 999;

    static int allocate(void **p, size_t bytes) {
        ++allocations; log += 'A';
        if (fail_allocation_in && --fail_allocation_in == 0) return kNoMemory;
        *p = std::malloc(bytes ? bytes : 1);
        outstanding.insert(*p);
        return 0;
    }
    static int release(void *p) {
        ++frees; log += 'F';
        if (!outstanding.erase(p)) { std::fprintf(stderr, "table_cache_check: free of a block that is not outstanding\n"); std::abort(); }
        freed.push_back(p);
        std::free(p);
        return 0;
    }
    static int copy(void *dst, const void *host, size_t bytes) {
        ++copies; log += 'C';
        if (fail_copy_in && --fail_copy_in == 0) return kCopyFailed;
        if (!outstanding.count(dst)) { std::fprintf(stderr, "table_cache_check: copy into a block that is not outstanding\n"); std::abort(); }
        std::memcpy(dst, host, bytes);
        return 0;
    }
    static void reset() {
        for (void *p : outstanding) std::free(p);
        outstanding.clear(); freed.clear(); log.clear();
        allocations = frees = copies = fail_allocation_in = fail_copy_in = 0;
    }
    static int calls() { return allocations + frees + copies; }
};

// An entry as lfg_internal.hpp's are: a key, the one allocation, a view into it and a host-side fact.
struct Entry {
    int in = 0, out = 0;
    std::pair<int, int> key() const { return {in, out}; }
    uint8_t *d_base = nullptr;
    const int32_t *view = nullptr;
    int fact = 0;
    bool operator==(const Entry &o) const { return in == o.in && out == o.out && d_base == o.d_base && view == o.view && fact == o.fact; }
};
using Cache = lfg::TableCache<Entry, Fake>;

int g_builds = 0, g_before_free = 0;
const auto before_free = [] { ++g_before_free; Fake::log += 'S'; };

// What every build_*_table of lfg_capi.cpp does: find, or build on the host, upload, set the views, insert.
lfg::DeviceStatus lookup(Cache &cache, int in, int out, Entry *got) {
    if (const auto hit = cache.find(std::make_pair(in, out))) { *got = *hit; return {}; }
    ++g_builds;
    const std::vector<int32_t> host = {in, out, in + out, 7};
    Entry e;
    e.in = in; e.out = out; e.fact = in * 1000 + out;
    const lfg::DeviceStatus s = lfg::upload<Fake>(host.data(), host.size() * sizeof(int32_t), &e.d_base);
    if (!s.ok()) return s;
    e.view = reinterpret_cast<const int32_t *>(e.d_base) + 2;
    cache.insert(e);
    *got = e;
    return {};
}

// The block is allocated and holds what was uploaded for (in, out): under the sanitizer a freed one is a report.
bool live(const Entry &e) { return Fake::outstanding.count(e.d_base) && *e.view == e.in + e.out && e.fact == e.in * 1000 + e.out; }

void fill(Cache &cache, int n) {                                   // keys (1, 101) .. (n, 100 + n), oldest first
    Entry e;
    for (int k = 1; k <= n; ++k) (void)lookup(cache, k, 100 + k, &e);
}

int g_checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        ++g_checks;                                                                                  \
        if (!(cond)) { std::printf("%s:%d: %s\n", __func__, __LINE__, #cond); std::exit(1); }      \
    } while (0)

void fresh() { Fake::reset(); g_builds = g_before_free = 0; }

void hit_touches_nothing() {
    fresh();
    Cache cache;
    Entry first, again;
    CHECK(lookup(cache, 1920, 3840, &first).ok());
    CHECK(Fake::allocations == 1 && Fake::copies == 1 && Fake::frees == 0 && Fake::log == "AC");
    const int calls = Fake::calls();
    CHECK(lookup(cache, 1920, 3840, &again).ok());
    CHECK(again == first && live(again));
    CHECK(Fake::calls() == calls && g_builds == 1);
    CHECK(!cache.find(std::make_pair(3840, 1920)) && Fake::calls() == calls);     // a miss of find alone touches nothing either
    cache.release_all();
}

void two_on_top_of_the_kept_stay_until_trim() {
    fresh();
    Cache cache;
    CHECK(Cache::kKeep == 14);
    fill(cache, 14);
    cache.trim(before_free);                                        // 14 held: nothing to do
    CHECK(g_before_free == 0 && Fake::frees == 0 && cache.size() == 14);
    Entry a, b;
    CHECK(lookup(cache, 15, 115, &a).ok() && lookup(cache, 16, 116, &b).ok());
    CHECK(cache.size() == 16 && Fake::frees == 0);
    for (int k = 1; k <= 16; ++k) {
        const auto e = cache.find(std::make_pair(k, 100 + k));
        CHECK(e && live(*e));
    }
    cache.release_all();
}

void trim_frees_the_oldest_in_order_after_one_wait() {
    fresh();
    Cache cache;
    fill(cache, 16);
    const Entry first = *cache.find(std::make_pair(1, 101)), second = *cache.find(std::make_pair(2, 102));
    Fake::log.clear();
    cache.trim(before_free);
    CHECK(g_before_free == 1 && Fake::log == "SFF");
    CHECK(Fake::freed.size() == 2 && Fake::freed[0] == first.d_base && Fake::freed[1] == second.d_base);
    CHECK(cache.size() == 14 && !cache.find(std::make_pair(1, 101)) && !cache.find(std::make_pair(2, 102)));
    for (int k = 3; k <= 16; ++k) CHECK(live(*cache.find(std::make_pair(k, 100 + k))));
    cache.trim(before_free);                                        // and again: nothing
    CHECK(g_before_free == 1 && Fake::frees == 2);
    cache.release_all();
}

void trim_on_few_does_nothing() {
    for (int n : {0, 1, 13, 14}) {
        fresh();
        Cache cache;
        fill(cache, n);
        const int calls = Fake::calls();
        cache.trim(before_free);
        CHECK(g_before_free == 0 && Fake::calls() == calls && cache.size() == (size_t)n);
        cache.release_all();
    }
}

// Round 3: a call whose first key is the oldest entry and whose second key is new.  Trim, lookup, lookup: both tables that
// the call was handed are still allocated when it launches, whether 14, 15 or 16 entries were held when it began.
void a_calls_two_lookups_cannot_free_each_other() {
    for (int held : {14, 15, 16}) {
        fresh();
        Cache cache;
        fill(cache, held);
        cache.trim(before_free);                                    // the top of the entry point
        const int oldest = held - 13;                               // the oldest entry that the trim kept
        Entry x, y;
        CHECK(lookup(cache, oldest, 100 + oldest, &x).ok());        // a hit on the oldest
        CHECK(lookup(cache, 77, 177, &y).ok());                     // a miss: built and inserted, the vector may move
        CHECK(live(x) && live(y) && cache.size() == 15);
        CHECK(g_before_free == (held > 14 ? 1 : 0));
        // the next call's trim may drop x's table (a hit has not refreshed its age) -- but only then
        cache.trim(before_free);
        CHECK(!cache.find(std::make_pair(oldest, 100 + oldest)) && live(y));
        cache.release_all();
    }
}

void an_evicted_key_is_built_again() {
    fresh();
    Cache cache;
    fill(cache, 15);
    CHECK(g_builds == 15);
    cache.trim(before_free);
    Entry e;
    CHECK(lookup(cache, 1, 101, &e).ok());
    CHECK(g_builds == 16 && Fake::allocations == 16 && Fake::copies == 16 && live(e));
    CHECK(lookup(cache, 1, 101, &e).ok() && g_builds == 16);
    cache.release_all();
}

void a_failed_upload_leaves_everything_as_it_was() {
    fresh();
    Cache cache;
    fill(cache, 3);
    const size_t blocks = Fake::outstanding.size();
    Entry e;
    e.fact = -1;
    Fake::fail_allocation_in = 1;
    lfg::DeviceStatus s = lookup(cache, 9, 109, &e);
    CHECK(!s.ok() && s.failed == lfg::DeviceStep::Allocate && s.error == Fake::kNoMemory);
    CHECK(cache.size() == 3 && Fake::outstanding.size() == blocks && !cache.find(std::make_pair(9, 109)) && e.fact == -1);
    CHECK(Fake::copies == 3 && Fake::frees == 0);                   // no copy into nothing, nothing to free
    Fake::fail_copy_in = 1;
    s = lookup(cache, 9, 109, &e);
    CHECK(!s.ok() && s.failed == lfg::DeviceStep::Copy && s.error == Fake::kCopyFailed);
    CHECK(cache.size() == 3 && Fake::outstanding.size() == blocks && !cache.find(std::make_pair(9, 109)) && e.fact == -1);
    CHECK(Fake::frees == 1);                                        // the allocation of the failed copy
    uint8_t *published = nullptr;                                   // the one-off tables: no pointer on failure
    const int32_t word = 5;
    Fake::fail_copy_in = 1;
    CHECK(!lfg::upload<Fake>(&word, sizeof word, &published).ok() && published == nullptr);
    CHECK(lookup(cache, 9, 109, &e).ok() && live(e) && cache.size() == 4);      // and the next attempt succeeds
    cache.release_all();
}

void release_all_leaves_nothing() {
    fresh();
    Cache cache;
    fill(cache, 16);
    cache.trim(before_free);
    cache.release_all();
    CHECK(Fake::outstanding.empty() && Fake::frees == 16 && Fake::allocations == 16 && cache.size() == 0);
    cache.release_all();                                            // (a double free would have aborted)
    CHECK(Fake::frees == 16);
}

int g_synchronized = 0, g_synchronize_error = 0;
const auto synchronize = [] { ++g_synchronized; Fake::log += 'S'; return g_synchronize_error; };

void lane_buffer() {
    fresh();
    g_synchronized = g_synchronize_error = 0;
    lfg::DeviceBuffer b;
    CHECK(lfg::grow<Fake>(b, 0, synchronize).ok() && Fake::calls() == 0 && g_synchronized == 0);      // need <= have, from nothing
    CHECK(lfg::grow<Fake>(b, 100, synchronize).ok());
    CHECK(b.data && b.bytes == 100 && Fake::log == "SA" && Fake::outstanding.count(b.data));
    CHECK(b.as<uint32_t>() == reinterpret_cast<uint32_t *>(b.data));
    uint8_t *const first = b.data;
    for (size_t need : {(size_t)100, (size_t)99, (size_t)1, (size_t)0}) {
        CHECK(lfg::grow<Fake>(b, need, synchronize).ok());
        CHECK(b.data == first && b.bytes == 100 && Fake::log == "SA" && g_synchronized == 1);        // nothing at all
    }
    Fake::log.clear();
    CHECK(lfg::grow<Fake>(b, 101, synchronize).ok());
    CHECK(Fake::log == "SFA" && Fake::freed.size() == 1 && Fake::freed[0] == first);                 // synchronise, then free, then allocate
    CHECK(b.bytes == 101 && Fake::outstanding.size() == 1 && Fake::outstanding.count(b.data));
    g_synchronize_error = 7;                                        // a failed wait: the buffer stays, nothing is freed
    Fake::log.clear();
    lfg::DeviceStatus s = lfg::grow<Fake>(b, 500, synchronize);
    CHECK(!s.ok() && s.failed == lfg::DeviceStep::Synchronize && s.error == 7 && Fake::log == "S" && b.bytes == 101 && Fake::outstanding.count(b.data));
    g_synchronize_error = 0;
    Fake::fail_allocation_in = 1;
    s = lfg::grow<Fake>(b, 500, synchronize);
    CHECK(!s.ok() && s.failed == lfg::DeviceStep::Allocate && s.error == Fake::kNoMemory);
    CHECK(b.data == nullptr && b.bytes == 0 && Fake::outstanding.empty());                            // {nullptr, 0}
    CHECK(lfg::grow<Fake>(b, 50, synchronize).ok() && b.bytes == 50);                                 // and it can grow again, from nothing
    const int frees = Fake::frees;
    lfg::release<Fake>(b);
    CHECK(b.data == nullptr && b.bytes == 0 && Fake::frees == frees + 1 && Fake::outstanding.empty());
    lfg::release<Fake>(b);                                          // twice is harmless
    CHECK(Fake::frees == frees + 1);
    lfg::DeviceBuffer copy = b;                                     // plain data: copied and reset as lfg_lane_state is
    copy = lfg::DeviceBuffer{};
    CHECK(copy.data == nullptr && copy.bytes == 0);
}

}  // namespace

int main() {
    hit_touches_nothing();
    two_on_top_of_the_kept_stay_until_trim();
    trim_frees_the_oldest_in_order_after_one_wait();
    trim_on_few_does_nothing();
    a_calls_two_lookups_cannot_free_each_other();
    an_evicted_key_is_built_again();
    a_failed_upload_leaves_everything_as_it_was();
    release_all_leaves_nothing();
    lane_buffer();
    Fake::reset();
    std::printf("ok %d\n", g_checks);
    return 0;
}
