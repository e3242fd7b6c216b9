// HIP on the host: a stand-in for <hip/hip_runtime.h> that lets g++ compile a csrc/*.hip file as it is (-x c++, this
// directory's parent in front of ROCm's on the include path, -ffp-contract=off as the library has it) and run its own
// launch_* function on the CPU: under -fsanitize=address,undefined every byte a kernel reads or writes outside a frame
// that ends where it ends is reported, under -fsanitize=thread every LDS cell read without the barrier that orders it.
// tests/cpp/hip_on_host_check.cpp holds every stand-in below to a plain definition; DESIGN.md section 4.10 says which kernel
// files run this way, which do not, and what such a run cannot show.
//
//   launching    hipLaunchKernelGGL runs the grid here, one block after another.  Lanes are a plain loop (the default: a
//                barrier or a cross-lane operation then aborts with a message), or, inside a hip_on_host::LaneThreads
//                scope, one thread each from a pool that lives as long as the program; a lane is threadIdx.x + blockDim.x *
//                (threadIdx.y + blockDim.y * threadIdx.z), a wave 64 consecutive lanes.  __shared__ is a static object:
//                zero at program start, and it keeps what the block before left.
//   barrier      __syncthreads() waits for every lane of the block that has not returned from the kernel.
//   cross-lane   ballot, __shfl_xor / __shfl_down, readlane, readfirstlane, update_dpp: a rendezvous of the wave's lanes
//                that have not returned, through an exchange array; each returns what the instruction returns on the
//                device.  A lane that has returned is what EXEC masks out there: it is not counted by a ballot, a shuffle
//                reads 0 from it, a DPP move treats it as a missing source, and readlane of it aborts (the device would hand
//                out a stale register).  Divergent lanes that have NOT returned are not modelled: every live lane of the
//                wave must arrive (a wait of 120 s aborts with a message).
//   arithmetic   v_sad_u8, v_cvt_pk_u8_f32 (round half to even, saturating, NaN -> 0: as measured, csrc/lfg_device.hpp),
//                v_perm_b32, v_dot4_u32_u8, __umul24, atomicMin / atomicAdd on 32- and 64-bit words, __ffsll, __popcll, min, max.
#pragma once

#ifndef LFG_ON_HOST
#define LFG_ON_HOST 1
#endif

#include <atomic>
#include <cmath>
#include <condition_variable>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static

struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct uint2 { unsigned x, y; };
struct uint4 { unsigned x, y, z, w; };
struct int2 { int x, y; };
struct float2 { float x, y; };
struct float4 { float x, y, z, w; };

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
typedef struct hip_on_host_stream *hipStream_t;
typedef struct hip_on_host_event *hipEvent_t;

inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipMalloc(void **p, size_t bytes) { *p = malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
inline hipError_t hipFree(void *p) { free(p); return hipSuccess; }
inline hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
inline hipError_t hipMemsetAsync(void *p, int value, size_t bytes, hipStream_t) { memset(p, value, bytes); return hipSuccess; }

inline thread_local dim3 threadIdx(0, 0, 0), blockIdx(0, 0, 0), blockDim, gridDim;

namespace hip_on_host {

[[noreturn]] inline void fail(const char *what) {
    fprintf(stderr, "hip_on_host: %s\n", what);
    fflush(stderr);
    abort();
}

// A barrier that a lane can leave for good.  The counters change under a mutex held for a few instructions; the lanes that
// wait spin on the generation and yield (a condition variable's wake of 255 threads costs far more than the kernels do).
class Barrier {
public:
    void reset(int lanes) { expected_ = lanes; arrived_ = 0; }
    void arrive_and_wait() {
        unsigned g;
        {
            std::lock_guard<std::mutex> lock(m_);
            g = generation_.load(std::memory_order_relaxed);
            if (++arrived_ == expected_) { release(); return; }
        }
        const auto start = std::chrono::steady_clock::now();
        for (unsigned spins = 1; generation_.load(std::memory_order_acquire) == g; ++spins) {
            if (spins % 64 == 0) std::this_thread::yield();
            if (spins % (1u << 20) == 0 && std::chrono::steady_clock::now() - start > std::chrono::seconds(120))
                fail("a barrier or a cross-lane operation that not every live lane reaches (120 s)");
        }
    }
    // `leaving` runs under the mutex, before the lanes that wait are let go
    template <typename F>
    void arrive_and_drop(F leaving) {
        std::lock_guard<std::mutex> lock(m_);
        leaving();
        --expected_;
        if (expected_ > 0 && arrived_ == expected_) release();
    }
    std::function<void()> on_release;          // under the mutex, before anyone is let go
private:
    void release() {
        arrived_ = 0;
        if (on_release) on_release();
        generation_.store(generation_.load(std::memory_order_relaxed) + 1, std::memory_order_release);
    }
    std::mutex m_;
    int expected_ = 0, arrived_ = 0;
    std::atomic<unsigned> generation_{0};
};

// A wave's rendezvous.  Operation k leaves its values in exchange[k % 2] and reads them behind ONE barrier: a lane can be at
// most one operation ahead of the slowest, so the other half is free.  liveAt[k % 2] is `live` as the barrier's release found
// it: the lanes that took part, whatever returns afterwards.
struct Wave {
    Barrier barrier;
    uint64_t live = 0;            // bit l: lane l of the wave has not returned (changed under the barrier's mutex)
    unsigned round = 0;           // operations released so far (under the barrier's mutex)
    uint64_t liveAt[2] = {};
    uint64_t exchange[2][64] = {};
    Wave() { barrier.on_release = [this] { liveAt[round++ % 2] = live; }; }
};

struct Lane {                      // what a lane's thread knows of its place; null in a plain loop
    Barrier *block = nullptr;
    Wave *wave = nullptr;
    int id = 0;                    // within the wave
    unsigned round = 0;            // the wave's operations this lane has taken part in
    std::atomic<bool> *synced = nullptr;   // set by the first barrier or cross-lane operation of the launch
};
inline thread_local Lane t_lane;

inline bool g_laneThreads = false;
// Inside this scope a launch may give every lane a thread: a kernel's first launch does, and where no lane met a barrier or
// a cross-lane operation in it, the kernel's later launches are plain loops (and abort with a message if one then does).
struct LaneThreads {
    bool before;
    explicit LaneThreads(bool on = true) : before(g_laneThreads) { g_laneThreads = on; }
    ~LaneThreads() { g_laneThreads = before; }
};

// The pool: worker i is lane i of every block of a launch.  Workers are made when a launch first needs them and joined
// when the program ends.
class Pool {
public:
    static Pool &get() { static Pool p; return p; }
    // body(lane) runs the whole grid for that lane
    void run(int lanes, const std::function<void(int)> &body) {
        while ((int)workers_.size() < lanes) {
            const int i = (int)workers_.size();
            workers_.emplace_back([this, i] { work(i); });
        }
        {
            std::lock_guard<std::mutex> lock(m_);
            body_ = &body; lanes_ = lanes; pending_ = lanes; ++job_;
        }
        start_.notify_all();
        std::unique_lock<std::mutex> lock(m_);
        done_.wait(lock, [&] { return pending_ == 0; });
        body_ = nullptr;
    }
    ~Pool() {
        { std::lock_guard<std::mutex> lock(m_); quit_ = true; ++job_; }
        start_.notify_all();
        for (auto &w : workers_) w.join();
    }
private:
    void work(int i) {
        unsigned seen = 0;
        for (;;) {
            const std::function<void(int)> *body;
            {
                std::unique_lock<std::mutex> lock(m_);
                start_.wait(lock, [&] { return job_ != seen; });
                seen = job_;
                if (quit_) return;
                if (i >= lanes_) continue;
                body = body_;
            }
            (*body)(i);
            std::lock_guard<std::mutex> lock(m_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable start_, done_;
    std::vector<std::thread> workers_;
    const std::function<void(int)> *body_ = nullptr;
    int lanes_ = 0, pending_ = 0;
    unsigned job_ = 0;
    bool quit_ = false;
};

inline void set_indices(const dim3 &grid, const dim3 &block, unsigned b, unsigned l) {
    gridDim = grid; blockDim = block;
    blockIdx = dim3(b % grid.x, b / grid.x % grid.y, b / grid.x / grid.y);
    threadIdx = dim3(l % block.x, l / block.x % block.y, l / block.x / block.y);
}

template <typename... Params, typename... Args>
void launch(void (*kernel)(Params...), dim3 grid, dim3 block, Args... args) {
    const unsigned blocks = grid.x * grid.y * grid.z, lanes = block.x * block.y * block.z;
    if (blocks == 0 || lanes == 0 || lanes > 1024) fail("a launch of no blocks, no lanes or more than 1024 lanes");
    static std::map<void *, bool> learnt;          // kernel -> some lane of its first threaded launch synchronised
    const auto known = learnt.find((void *)kernel);
    if (!g_laneThreads || (known != learnt.end() && !known->second)) {
        for (unsigned b = 0; b < blocks; ++b)
            for (unsigned l = 0; l < lanes; ++l) {
                set_indices(grid, block, b, l);
                kernel(static_cast<Params>(args)...);
            }
        return;
    }
    const unsigned waves = (lanes + 63) / 64;
    Barrier blockBarrier, between;          // between: every lane has left block b before one enters block b + 1
    std::unique_ptr<Wave[]> wave(new Wave[waves]);
    auto arm = [&] {
        blockBarrier.reset((int)lanes);
        for (unsigned w = 0; w < waves; ++w) {
            const unsigned n = w + 1 < waves ? 64u : lanes - 64u * w;
            wave[w].barrier.reset((int)n);
            wave[w].live = n == 64 ? ~0ull : (1ull << n) - 1;
            wave[w].round = 0;
        }
    };
    std::atomic<bool> synced{false};
    arm();
    between.reset((int)lanes);
    const std::function<void(int)> body = [&](int l) {
        for (unsigned b = 0; b < blocks; ++b) {
            set_indices(grid, block, b, (unsigned)l);
            Wave *w = &wave[l / 64];
            t_lane = Lane{&blockBarrier, w, l % 64, 0u, &synced};
            kernel(static_cast<Params>(args)...);
            t_lane = Lane{};
            w->barrier.arrive_and_drop([&] { w->live &= ~(1ull << (l % 64)); });
            blockBarrier.arrive_and_drop([] {});
            between.arrive_and_wait();
            if (l == 0) arm();
            between.arrive_and_wait();
        }
    };
    Pool::get().run((int)lanes, body);
    learnt[(void *)kernel] = (known != learnt.end() && known->second) || synced.load();
}

inline Lane &lane_or_fail(const char *what) {
    if (!t_lane.block) {
        fprintf(stderr, "hip_on_host: %s in a launch whose lanes are a plain loop: outside hip_on_host::LaneThreads, or in a kernel "
                        "whose first launch met none\n", what);
        abort();
    }
    if (!t_lane.synced->load(std::memory_order_relaxed)) t_lane.synced->store(true, std::memory_order_relaxed);
    return t_lane;
}

// One rendezvous: every live lane of the wave leaves `mine`, then `read(exchange, live, lane)` runs in each.
template <typename F>
inline auto exchange(const char *what, uint64_t mine, F read) {
    Lane &me = lane_or_fail(what);
    const unsigned half = me.round++ % 2;
    me.wave->exchange[half][me.id] = mine;
    me.wave->barrier.arrive_and_wait();
    return read(me.wave->exchange[half], me.wave->liveAt[half], me.id);
}

// The source lane of a DPP control word for lane l, -1 where there is none.  The control words the kernels in scope use.
inline int dpp_source(int ctrl, int l) {
    const int row = l & ~15, in = l & 15;
    if (ctrl >= 0x00 && ctrl <= 0xFF) return (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);                 // quad_perm
    if (ctrl >= 0x101 && ctrl <= 0x10F) return in + (ctrl & 15) <= 15 ? l + (ctrl & 15) : -1;          // row_shl
    if (ctrl >= 0x111 && ctrl <= 0x11F) return in - (ctrl & 15) >= 0 ? l - (ctrl & 15) : -1;           // row_shr
    if (ctrl == 0x130) return l + 1 <= 63 ? l + 1 : -1;                                                // wave_shl:1
    if (ctrl == 0x138) return l - 1 >= 0 ? l - 1 : -1;                                                 // wave_shr:1
    if (ctrl == 0x140) return row | (15 - in);                                                         // row_mirror
    if (ctrl == 0x141) return (l & ~7) | (7 - (l & 7));                                                // row_half_mirror
    if (ctrl == 0x142) return row >= 16 ? row - 1 : -1;                                                // row_bcast15
    if (ctrl == 0x143) return row >= 32 ? 31 : -1;                                                     // row_bcast31
    fprintf(stderr, "hip_on_host: update_dpp control word 0x%X has no stand-in\n", ctrl);
    abort();
}

}  // namespace hip_on_host

template <typename... Params, typename... Args>
inline void hipLaunchKernelGGL(void (*kernel)(Params...), dim3 grid, dim3 block, size_t, hipStream_t, Args... args) {
    hip_on_host::launch(kernel, grid, block, args...);
}

inline void __syncthreads() { hip_on_host::lane_or_fail("__syncthreads()").block->arrive_and_wait(); }

// ---- cross-lane
inline uint64_t __builtin_amdgcn_ballot_w64(bool p) {
    return hip_on_host::exchange("a ballot", p ? 1u : 0u, [](const uint64_t *x, uint64_t live, int) {
        uint64_t m = 0;
        for (int l = 0; l < 64; ++l) if (((live >> l) & 1u) && x[l]) m |= 1ull << l;
        return m;
    });
}
inline uint64_t __ballot(int p) { return __builtin_amdgcn_ballot_w64(p != 0); }

namespace hip_on_host {
template <typename T> inline uint64_t to_bits(T v) { uint64_t b = 0; static_assert(sizeof(T) <= 8, ""); memcpy(&b, &v, sizeof(T)); return b; }
template <typename T> inline T from_bits(uint64_t b) { T v; memcpy(&v, &b, sizeof(T)); return v; }
}

// ds_bpermute: a source that has returned reads as 0; width splits the wave into groups that do not see each other.
template <typename T>
inline T __shfl_xor(T v, int mask, int width = 64) {
    return hip_on_host::from_bits<T>(hip_on_host::exchange("__shfl_xor", hip_on_host::to_bits(v), [=](const uint64_t *x, uint64_t live, int me) {
        int src = me ^ mask;
        if (src / width != me / width || src > 63) src = me;
        return ((live >> src) & 1u) ? x[src] : 0ull;
    }));
}
template <typename T>
inline T __shfl_down(T v, unsigned delta, int width = 64) {
    return hip_on_host::from_bits<T>(hip_on_host::exchange("__shfl_down", hip_on_host::to_bits(v), [=](const uint64_t *x, uint64_t live, int me) {
        int src = me + (int)delta;
        if (src / width != me / width || src > 63) src = me;
        return ((live >> src) & 1u) ? x[src] : 0ull;
    }));
}
inline int __builtin_amdgcn_readlane(int v, int lane) {
    return (int)(uint32_t)hip_on_host::exchange("readlane", (uint32_t)v, [=](const uint64_t *x, uint64_t live, int) {
        if (lane < 0 || lane > 63 || !((live >> lane) & 1u)) hip_on_host::fail("readlane of a lane that has returned: a stale register on the device");
        return x[lane];
    });
}
inline int __builtin_amdgcn_readfirstlane(int v) {
    return (int)(uint32_t)hip_on_host::exchange("readfirstlane", (uint32_t)v, [](const uint64_t *x, uint64_t live, int) {
        return x[__builtin_ctzll(live)];
    });
}
inline int __builtin_amdgcn_update_dpp(int old, int src, int ctrl, int rowMask, int bankMask, bool boundCtrl) {
    return (int)(uint32_t)hip_on_host::exchange("update_dpp", (uint32_t)src, [=](const uint64_t *x, uint64_t live, int me) -> uint64_t {
        const int s = hip_on_host::dpp_source(ctrl, me);
        if (!((rowMask >> (me >> 4)) & 1) || !((bankMask >> ((me >> 2) & 3)) & 1)) return (uint32_t)old;
        if ((ctrl == 0x142 || ctrl == 0x143) && boundCtrl) hip_on_host::fail("update_dpp: a row broadcast with bound_ctrl has no stand-in");
        if (s < 0 || !((live >> s) & 1u)) return boundCtrl ? 0u : (uint32_t)old;
        return x[s];
    });
}

// ---- arithmetic
inline uint32_t __builtin_amdgcn_sad_u8(uint32_t a, uint32_t b, uint32_t acc) {
    for (int k = 0; k < 4; ++k) {
        const int x = (int)((a >> (8 * k)) & 0xffu), y = (int)((b >> (8 * k)) & 0xffu);
        acc += (uint32_t)(x > y ? x - y : y - x);
    }
    return acc;
}
// byte `sel` of `old` replaced by the float as a byte: round half to even, saturating, NaN -> 0
inline uint32_t __builtin_amdgcn_cvt_pk_u8_f32(float v, uint32_t sel, uint32_t old) {
    uint32_t b;
    if (!(v == v)) b = 0u;
    else if (v <= 0.0f) b = 0u;
    else if (v >= 255.0f) b = 255u;
    else {
        const float f = __builtin_floorf(v), r = v - f;
        b = (uint32_t)f;
        if (r > 0.5f || (r == 0.5f && (b & 1u))) ++b;
    }
    const uint32_t shift = 8u * (sel & 3u);
    return (old & ~(0xffu << shift)) | (b << shift);
}
// v_perm_b32: byte k of the result is byte sel_k of {a (bytes 7..4), b (bytes 3..0)}; 12: 0x00, 13 and above: 0xFF
inline uint32_t __builtin_amdgcn_perm(uint32_t a, uint32_t b, uint32_t sel) {
    const uint64_t both = ((uint64_t)a << 32) | b;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = (sel >> (8 * k)) & 0xffu;
        uint32_t byte;
        if (s <= 7) byte = (uint32_t)(both >> (8 * s)) & 0xffu;
        else if (s == 12) byte = 0u;
        else if (s >= 13) byte = 0xffu;
        else hip_on_host::fail("v_perm_b32 selector 8 .. 11 (sign bytes) has no stand-in");
        r |= byte << (8 * k);
    }
    return r;
}
inline uint32_t __builtin_amdgcn_udot4(uint32_t a, uint32_t b, uint32_t acc, bool clamp) {
    if (clamp) hip_on_host::fail("udot4 with clamp has no stand-in");
    for (int k = 0; k < 4; ++k) acc += ((a >> (8 * k)) & 0xffu) * ((b >> (8 * k)) & 0xffu);
    return acc;
}
inline uint32_t __umul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __popc(unsigned v) { return __builtin_popcount(v); }

template <typename T>
inline T hip_on_host_atomic_min(T *p, T v) {
    T seen = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < seen && !__atomic_compare_exchange_n(p, &seen, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return seen;
}
inline uint32_t atomicMin(uint32_t *p, uint32_t v) { return hip_on_host_atomic_min(p, v); }
inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { return hip_on_host_atomic_min(p, v); }
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned min(unsigned a, unsigned b) { return a < b ? a : b; }
inline unsigned max(unsigned a, unsigned b) { return a > b ? a : b; }
inline long long min(long long a, long long b) { return a < b ? a : b; }
inline long long max(long long a, long long b) { return a > b ? a : b; }
inline unsigned long long min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
inline unsigned long long max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
inline unsigned long min(unsigned long a, unsigned long b) { return a < b ? a : b; }
inline unsigned long max(unsigned long a, unsigned long b) { return a > b ? a : b; }
inline float min(float a, float b) { return __builtin_fminf(a, b); }
inline float max(float a, float b) { return __builtin_fmaxf(a, b); }

// csrc/lfg_device.hpp's 16-byte store (its device form is inline assembly, left out under LFG_ON_HOST): the alignment the
// instruction needs is checked, the range is the sanitizer's.
namespace lfg {
inline void store_16_guarded(uint8_t *p, uint4 q) {
    if ((uintptr_t)p % 16) hip_on_host::fail("a 16-byte store to an address that is not 16-byte aligned");
    memcpy(p, &q, 16);
}
}  // namespace lfg
