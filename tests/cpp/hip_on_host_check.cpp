// tests/cpp/hip_on_host/hip/hip_runtime.h held to plain definitions, before anything that runs a kernel through it is believed:
// the arithmetic stand-ins over all byte pairs and the table csrc/lfg_device.hpp records, the index arithmetic of a launch in
// both lane modes, every cross-lane primitive on random lane values with all lanes live and with lanes that have returned (a
// ragged tail, and a ragged head and tail), a barrier that returned lanes have left, and the atomics from 256 lanes.  The
// expected values are written as scatters from the source lanes or as loops over the wave, never by calling the layer.
// Prints "ok <checks>"; tests/test_hip_on_host.py builds it plainly and with -fsanitize=address,undefined.
#include <hip/hip_runtime.h>

#include <cmath>
#include <random>

static long g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// ---- arithmetic
static void arithmetic() {
    for (unsigned a = 0; a < 256; ++a)
        for (unsigned b = 0; b < 256; ++b) {
            const unsigned d = a > b ? a - b : b - a;
            for (int k = 0; k < 4; ++k) CHECK(__builtin_amdgcn_sad_u8(a << (8 * k), b << (8 * k), 7u) == d + 7u);
            CHECK(__builtin_amdgcn_sad_u8(a * 0x01010101u, b * 0x01010101u, 0u) == 4 * d);
            CHECK(__builtin_amdgcn_sad_u8(a | (b << 16), b | (a << 16), 1000u) == 2 * d + 1000u);
            // cvt_pk: byte a into each position of a word of b's: the other bytes stay
            for (unsigned sel = 0; sel < 4; ++sel) {
                const uint32_t old = b * 0x01010101u, got = __builtin_amdgcn_cvt_pk_u8_f32((float)a, sel, old);
                CHECK(got == ((old & ~(0xffu << (8 * sel))) | (a << (8 * sel))));
            }
            CHECK(__builtin_amdgcn_udot4(a * 0x01010101u, b | (b << 16), 5u, false) == 2 * a * b + 5u);
        }
    // the table of lfg_device.hpp, then round half to even and saturation on a grid of 64ths (nearbyintf rounds half to even)
    const float in[] = {0.5f, 1.5f, 2.5f, 254.5f, 300.0f, -3.0f};
    const uint32_t out[] = {0, 2, 2, 254, 255, 0};
    for (int i = 0; i < 6; ++i) CHECK(__builtin_amdgcn_cvt_pk_u8_f32(in[i], 0u, 0u) == out[i]);
    for (int i = -4 * 64; i <= 260 * 64; ++i) {
        const float v = (float)i / 64.0f;
        const float want = std::fmin(std::fmax(std::nearbyintf(v), 0.0f), 255.0f);
        CHECK(__builtin_amdgcn_cvt_pk_u8_f32(v, 0u, 0u) == (uint32_t)want);
    }
    CHECK(__builtin_amdgcn_cvt_pk_u8_f32(std::nanf(""), 1u, 0xffffffffu) == 0xffff00ffu);
    CHECK(__builtin_amdgcn_cvt_pk_u8_f32(INFINITY, 0u, 0u) == 255u && __builtin_amdgcn_cvt_pk_u8_f32(-INFINITY, 0u, 0xffu) == 0u);
    CHECK(__builtin_amdgcn_cvt_pk_u8_f32(std::nextafterf(0.5f, 1.0f), 0u, 0u) == 1u && __builtin_amdgcn_cvt_pk_u8_f32(std::nextafterf(1.5f, 0.0f), 0u, 0u) == 1u);
    CHECK(__builtin_amdgcn_perm(0x77665544u, 0x33221100u, 0x07040300u) == 0x77443300u);
    CHECK(__builtin_amdgcn_perm(0x77665544u, 0x33221100u, 0x0c0d0105u) == 0x00ff1155u);
    CHECK(__ffsll(0) == 0 && __ffsll(1) == 1 && __ffsll((long long)(1ull << 63)) == 64 && __ffsll(0x50) == 5);
    CHECK(__popcll(~0ull) == 64 && __popcll(0x8000000000000001ull) == 2);
    CHECK(__umul24(0x01000003u, 5u) == 15u);
    CHECK(min(3, -2) == -2 && max(3u, 7u) == 7u && min(~0ull, 5ull) == 5ull && max(-1.0f, 2.0f) == 2.0f);
}

// ---- a launch's indices, both modes: every (block, thread) once, with the dimensions it was launched with
static uint32_t *g_seen;
__global__ void index_kernel(int gx, int gy, int gz, int bx, int by, int bz) {
    const bool dims = (int)gridDim.x == gx && (int)gridDim.y == gy && (int)gridDim.z == gz && (int)blockDim.x == bx && (int)blockDim.y == by && (int)blockDim.z == bz;
    const bool inside = (int)blockIdx.x < gx && (int)blockIdx.y < gy && (int)blockIdx.z < gz && (int)threadIdx.x < bx && (int)threadIdx.y < by && (int)threadIdx.z < bz;
    if (!dims || !inside) return;
    const size_t b = blockIdx.x + (size_t)gx * (blockIdx.y + (size_t)gy * blockIdx.z), t = threadIdx.x + (size_t)bx * (threadIdx.y + (size_t)by * threadIdx.z);
    atomicAdd(&g_seen[b * (size_t)(bx * by * bz) + t], 1u);
}
static void indices() {
    for (int mode = 0; mode < 2; ++mode) {
        hip_on_host::LaneThreads scope(mode == 1);
        const int g[3] = {3, 2, 2}, b[3] = {5, 7, 3};
        std::vector<uint32_t> seen((size_t)3 * 2 * 2 * 5 * 7 * 3, 0u);
        g_seen = seen.data();
        hipLaunchKernelGGL(index_kernel, dim3(g[0], g[1], g[2]), dim3(b[0], b[1], b[2]), 0, nullptr, g[0], g[1], g[2], b[0], b[1], b[2]);
        for (uint32_t s : seen) CHECK(s == 1u);
    }
}

// ---- cross-lane.  Block of 256 lanes; lane l of the block is live where g_liveOf[l]; the others return at once.
constexpr int kLanes = 256;
static bool g_liveOf[kLanes];
static uint64_t g_val[kLanes];
enum Op { kBallot, kShflXor, kShflDown, kReadlane, kReadfirst, kDpp };
struct Request { Op op; int a, b, c; bool bound; };          // a: mask / delta / lane / ctrl, b: width / row mask, c: bank mask
static uint64_t g_out[kLanes];

__global__ void cross_kernel(Request r) {
    const int l = (int)(threadIdx.x + blockDim.x * threadIdx.y);
    if (!g_liveOf[l]) return;
    const uint64_t v = g_val[l];
    uint64_t out = 0;
    switch (r.op) {
        case kBallot: out = __builtin_amdgcn_ballot_w64((v & 1u) != 0); break;
        case kShflXor: out = __shfl_xor((unsigned long long)v, r.a, r.b); break;
        case kShflDown: out = __shfl_down((unsigned long long)v, (unsigned)r.a, r.b); break;
        case kReadlane: out = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, r.a); break;
        case kReadfirst: out = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v); break;
        case kDpp: out = (uint32_t)__builtin_amdgcn_update_dpp((int)0xD00DFEEDu, (int)(uint32_t)v, r.a, r.b, r.c, r.bound); break;
    }
    g_out[l] = out;
}

static void run_cross(Request r) {
    hip_on_host::LaneThreads scope;
    for (auto &o : g_out) o = 0x0BADull;
    hipLaunchKernelGGL(cross_kernel, dim3(1), dim3(64, kLanes / 64), 0, nullptr, r);
}

// What lane `dst` of a wave receives from a DPP move, as a scatter: every source lane s says where its value goes.
static void dpp_scatter(int ctrl, int (&from)[64]) {
    for (int &f : from) f = -1;
    for (int s = 0; s < 64; ++s) {
        const int row = s / 16, in = s % 16;
        auto put = [&](int d) { if (d >= 0 && d < 64) from[d] = s; };
        if (ctrl <= 0xFF) { for (int q = 0; q < 4; ++q) if (((ctrl >> (2 * q)) & 3) == s % 4) put(s / 4 * 4 + q); }
        else if (ctrl >= 0x101 && ctrl <= 0x10F) { if (in - (ctrl & 15) >= 0) put(s - (ctrl & 15)); }               // shl: towards lane 0
        else if (ctrl >= 0x111 && ctrl <= 0x11F) { if (in + (ctrl & 15) <= 15) put(s + (ctrl & 15)); }              // shr: away from lane 0
        else if (ctrl == 0x130) put(s - 1);
        else if (ctrl == 0x138) put(s + 1);
        else if (ctrl == 0x140) put(row * 16 + 15 - in);
        else if (ctrl == 0x141) put(s / 8 * 8 + 7 - s % 8);
        else if (ctrl == 0x142) { if (in == 15 && row < 3) for (int d = 0; d < 16; ++d) put((row + 1) * 16 + d); }
        else if (ctrl == 0x143) { if (s == 31) for (int d = 32; d < 64; ++d) put(d); }
    }
}

static void cross_lane(std::mt19937_64 &rng, int pattern) {
    // pattern 0: all live.  1: a ragged tail -- 155 live lanes: waves 0 and 1 whole, 27 lanes of wave 2, wave 3 gone.
    // 2: a ragged head and tail in every wave: lanes 5 .. 49 of each.
    for (int l = 0; l < kLanes; ++l) {
        g_liveOf[l] = pattern == 0 || (pattern == 1 ? l < 155 : (l % 64 >= 5 && l % 64 < 50));
        g_val[l] = rng();
    }
    auto live = [&](int w, int l) { return l >= 0 && l < 64 && g_liveOf[64 * w + l]; };
    auto each = [&](auto expect) {
        for (int l = 0; l < kLanes; ++l) {
            if (g_liveOf[l]) CHECK(g_out[l] == expect(l / 64, l % 64));
            else CHECK(g_out[l] == 0x0BADull);
        }
    };
    run_cross({kBallot, 0, 0, 0, false});
    each([&](int w, int) { uint64_t m = 0; for (int k = 0; k < 64; ++k) if (live(w, k) && (g_val[64 * w + k] & 1u)) m |= 1ull << k; return m; });
    for (int width : {64, 16})
        for (int mask = 1; mask < width; mask <<= 1) {
            run_cross({kShflXor, mask, width, 0, false});
            each([&](int w, int l) { return live(w, l ^ mask) ? g_val[64 * w + (l ^ mask)] : 0ull; });
        }
    for (int delta : {1, 3, 32}) {
        run_cross({kShflDown, delta, 64, 0, false});
        each([&](int w, int l) { const int s = l + delta < 64 ? l + delta : l; return live(w, s) ? g_val[64 * w + s] : 0ull; });
    }
    run_cross({kShflDown, 2, 8, 0, false});
    each([&](int w, int l) { const int s = l % 8 + 2 < 8 ? l + 2 : l; return live(w, s) ? g_val[64 * w + s] : 0ull; });
    for (int lane : {5, 17, 26}) {                                     // live in every pattern, in every wave that has a live lane
        run_cross({kReadlane, lane, 0, 0, false});
        each([&](int w, int) { return (uint64_t)(uint32_t)g_val[64 * w + lane]; });
    }
    run_cross({kReadfirst, 0, 0, 0, false});
    each([&](int w, int) { int f = 0; while (!live(w, f)) ++f; return (uint64_t)(uint32_t)g_val[64 * w + f]; });
    struct Move { int ctrl, rows; };
    const Move moves[] = {{0xB1, 0xF}, {0x4E, 0xF}, {0x1B, 0xF}, {0x141, 0xF}, {0x140, 0xF}, {0x142, 0xA}, {0x143, 0xC}, {0x101, 0xF}, {0x102, 0xF},
                          {0x104, 0xF}, {0x108, 0xF}, {0x111, 0xF}, {0x112, 0xF}, {0x114, 0xF}, {0x118, 0xF}, {0x130, 0xF}, {0x138, 0xF}, {0x111, 0x5}};
    for (const Move &m : moves)
        for (int bound = 0; bound < 2; ++bound)
            for (int banks : {0xF, 0x6}) {
                if (bound && (m.ctrl == 0x142 || m.ctrl == 0x143)) continue;
                int from[64];
                dpp_scatter(m.ctrl, from);
                run_cross({kDpp, m.ctrl, m.rows, banks, bound != 0});
                each([&](int w, int l) -> uint64_t {
                    if (!((m.rows >> (l / 16)) & 1) || !((banks >> (l % 16 / 4)) & 1)) return 0xD00DFEEDu;
                    if (from[l] < 0 || !live(w, from[l])) return bound ? 0u : 0xD00DFEEDu;
                    return (uint32_t)g_val[64 * w + from[l]];
                });
            }
}

// ---- a barrier that returned lanes have left, and LDS behind it; the atomics from every lane of several blocks
static uint32_t g_ring[kLanes];
static uint32_t g_min32, g_sum32;
static unsigned long long g_min64, g_sum64;
__global__ void barrier_kernel(int n, int rounds) {
    __shared__ uint32_t cell[kLanes];
    const int l = (int)threadIdx.x;
    if (l >= n) return;
    uint32_t carry = (uint32_t)g_val[l];
    for (int r = 0; r < rounds; ++r) {
        cell[l] = carry;
        __syncthreads();
        carry = cell[(l + 1) % n] + 1u;
        __syncthreads();
    }
    g_ring[l] = carry;
}
__global__ void atomic_kernel() {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t v = (i * 2654435761u) >> 7;
    atomicMin(&g_min32, v);
    atomicMin(&g_min64, ((unsigned long long)v << 20) | i);
    atomicAdd(&g_sum32, v & 0xffu);
    atomicAdd(&g_sum64, (unsigned long long)v << 8);
}
static void barrier_and_atomics() {
    hip_on_host::LaneThreads scope;
    for (int n : {kLanes, 155, 1}) {
        for (auto &r : g_ring) r = 0x0BADu;
        hipLaunchKernelGGL(barrier_kernel, dim3(2), dim3(kLanes), 0, nullptr, n, 5);
        for (int l = 0; l < kLanes; ++l) CHECK(g_ring[l] == (l < n ? (uint32_t)g_val[(l + 5) % n] + 5u : 0x0BADu));
    }
    g_min32 = ~0u; g_min64 = ~0ull; g_sum32 = 0; g_sum64 = 0;
    hipLaunchKernelGGL(atomic_kernel, dim3(3), dim3(kLanes), 0, nullptr);
    uint32_t min32 = ~0u, sum32 = 0;
    unsigned long long min64 = ~0ull, sum64 = 0;
    for (uint32_t i = 0; i < 3 * kLanes; ++i) {
        const uint32_t v = (i * 2654435761u) >> 7;
        min32 = v < min32 ? v : min32;
        const unsigned long long k = ((unsigned long long)v << 20) | i;
        min64 = k < min64 ? k : min64;
        sum32 += v & 0xffu;
        sum64 += (unsigned long long)v << 8;
    }
    CHECK(g_min32 == min32 && g_min64 == min64 && g_sum32 == sum32 && g_sum64 == sum64);
}

int main() {
    std::mt19937_64 rng(20240607);
    arithmetic();
    indices();
    for (int pattern = 0; pattern < 3; ++pattern) cross_lane(rng, pattern);
    barrier_and_atomics();
    printf("ok %ld\n", g_checks);
    return 0;
}
