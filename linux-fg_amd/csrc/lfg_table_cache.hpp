// Context-owned device memory of the C-ABI layer (lfg_capi.cpp), free of HIP: the one upload of a finished host block, the one
// bounded cache of per-size tables, and the one grow-only buffer of a lane.  Standard library only, so that
// tests/cpp/table_cache_check.cpp holds every rule below to a counting fake with g++ alone.
//
// `Device` is a struct of three static functions that return 0 on success and the device's error code otherwise:
//     int allocate(void **p, size_t bytes);   int release(void *p);   int copy(void *dst, const void *host, size_t bytes);
// copy is synchronous: the host block may go out of scope as soon as it returns.  lfg_internal.hpp: HipDevice.
#pragma once

#include <cstddef>
#include <cstdint>
#include <optional>
#include <vector>

namespace lfg {

// Which step of upload() or grow() failed, and the device's code for it.
enum class DeviceStep { None, Synchronize, Allocate, Copy };
struct DeviceStatus {
    int error = 0;
    DeviceStep failed = DeviceStep::None;
    bool ok() const { return failed == DeviceStep::None; }
};

// One allocation of `bytes` and one synchronous copy of `host` into it.  *out is written on success only: on a failed copy
// the allocation is freed, so a caller never publishes a table that is half there.
template <class Device>
DeviceStatus upload(const void *host, size_t bytes, uint8_t **out) {
    void *d = nullptr;
    int e = Device::allocate(&d, bytes);
    if (e) return {e, DeviceStep::Allocate};
    e = Device::copy(d, host, bytes);
    if (e) { (void)Device::release(d); return {e, DeviceStep::Copy}; }
    *out = static_cast<uint8_t *>(d);
    return {};
}

// The tables of one kind that a context keeps, by key.  An Entry has key() (compared with ==), d_base (its ONE device
// allocation) and whatever views into that allocation and host-side facts the launchers need.
//
// The contract, stated here and nowhere else:
//   - find() returns a COPY of the entry and the cache never hands out a pointer or reference into its storage, so nothing a
//     caller holds moves when a later insert() grows the vector;
//   - what a copy points at on the device stays allocated until the next trim() or release_all().  An entry point calls trim()
//     once, at its top, before its first lookup: then the lookups of one call (width and height: two finds, two inserts at the
//     most) can never free each other's table, and kKeep entries are held between calls, kKeep + 2 within one;
//   - trim() drops the oldest first.  A hit does not refresh an entry's age;
//   - before_free() -- the wait for every lane, a queued kernel may still read what is about to go -- is called exactly once,
//     before the first free, and not at all when nothing is dropped.
template <class Entry, class Device>
class TableCache {
public:
    static constexpr size_t kKeep = 14;

    template <class Key>
    std::optional<Entry> find(const Key &key) const {
        for (const Entry &e : entries_)
            if (e.key() == key) return e;
        return std::nullopt;
    }
    void insert(const Entry &e) { entries_.push_back(e); }
    template <class BeforeFree>
    void trim(BeforeFree before_free) {
        if (entries_.size() <= kKeep) return;
        before_free();
        const size_t drop = entries_.size() - kKeep;
        for (size_t i = 0; i < drop; ++i) (void)Device::release(entries_[i].d_base);
        entries_.erase(entries_.begin(), entries_.begin() + (std::ptrdiff_t)drop);
    }
    void release_all() {
        for (const Entry &e : entries_) (void)Device::release(e.d_base);
        entries_.clear();
    }
    size_t size() const { return entries_.size(); }

private:
    std::vector<Entry> entries_;
};

// A device buffer that a lane owns and only ever grows.  Plain data with no destructor: lfg_lane_state is copied by value and
// reset by assignment, and lane_release frees what it lists.
struct DeviceBuffer {
    uint8_t *data = nullptr;
    size_t bytes = 0;
    template <class T>
    T *as() const { return reinterpret_cast<T *>(data); }
};

template <class Device>
void release(DeviceBuffer &b) {
    if (b.data) (void)Device::release(b.data);
    b = DeviceBuffer{};
}

// At least `need` bytes: nothing where the buffer is large enough; otherwise synchronize() (the lane's earlier calls may still
// use the old one), free, allocate.  The contents are not kept.  A failed allocation leaves {nullptr, 0}.
template <class Device, class Synchronize>
DeviceStatus grow(DeviceBuffer &b, size_t need, Synchronize synchronize) {
    if (need <= b.bytes) return {};
    int e = synchronize();
    if (e) return {e, DeviceStep::Synchronize};
    release<Device>(b);
    void *d = nullptr;
    e = Device::allocate(&d, need);
    if (e) return {e, DeviceStep::Allocate};
    b.data = static_cast<uint8_t *>(d);
    b.bytes = need;
    return {};
}

}  // namespace lfg
