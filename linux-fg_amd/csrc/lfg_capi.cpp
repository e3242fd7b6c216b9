// lfg_capi.cpp -- implementation of the C-ABI in include/linuxfg_hip.h.
// The only translation units that touch HIP are this file, lfg_comm.cpp and the kernel files (*.hip).
// There is no CPU fallback anywhere: every entry point needs a live HIP device.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "lfg_bicubic.hpp"
#include "lfg_deband.hpp"
#include "lfg_denoise.hpp"
#include "lfg_internal.hpp"
#include "lfg_levels.hpp"

#define LFG_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

std::string g_create_error;       // lfg_last_error(NULL)

int fail(lfg_context *ctx, int code, const std::string &msg) {
    if (ctx) ctx->error = msg; else g_create_error = msg;
    return code;
}

int fail_hip(lfg_context *ctx, hipError_t e, const char *what) {
    return fail(ctx, e == hipErrorOutOfMemory ? LFG_ERR_NOMEM : LFG_ERR_DEVICE,
                std::string(what) + ": " + hipGetErrorString(e));
}

#define LFG_HIP(ctx, call)                                            \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) return fail_hip((ctx), e_, #call);      \
    } while (0)

uint32_t bytes_per_pixel(uint32_t format) {
    switch (format) {
        case LFG_FORMAT_RGBA8_UNORM: return 4;
        case LFG_FORMAT_MV_S8X2: return 2;
        case LFG_FORMAT_MV_S16X2_Q2: return 4;
        default: return 0;
    }
}

// The largest lfg_frame pitch (include/linuxfg_hip.h): the frame kernels take the pitch as a 32-bit int.
constexpr uint32_t kMaxFramePitch = 0x7fffffffu;

// A frame whose pitch no call takes: NULL is not this function's to refuse.
bool pitch_too_large(const lfg_frame *f) { return f && f->pitch > kMaxFramePitch; }

bool frame_ok(const lfg_frame *f, uint32_t format) {
    return f && f->data && f->width > 0 && f->height > 0 && f->format == format && f->pitch <= kMaxFramePitch &&
           (uint64_t)f->pitch >= (uint64_t)f->width * bytes_per_pixel(format);
}

bool same_size(const lfg_frame *a, const lfg_frame *b) { return a->width == b->width && a->height == b->height; }

// ---- Lanczos tables: the per-axis part of shaders/scale.comp:16-41, same fp32 operation order.

float lanczos_ref(float x) {                                   // scale.comp:16-20
    if (x == 0.0f) return 1.0f;
    const float px = 3.14159265359f * x;
    const float s1 = (float)std::sin((double)px);
    const float s2 = (float)std::sin((double)(px / 3.0f));
    return 3.0f * s1 * s2 / (px * px);
}

// Everything the context has enqueued, on every lane (a resource shared by the lanes is about to go or to be read).
hipError_t sync_lanes(lfg_context *ctx) {
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < ctx->lanes.size() && e == hipSuccess; ++k) e = hipStreamSynchronize(ctx->from_selected(k).stream);
    return e;
}

// The one place that allocates and fills a device table (lfg_table_cache.hpp: upload): `what` names it in the error.
int upload_table(lfg_context *ctx, const void *host, size_t bytes, const char *what, uint8_t **out) {
    const lfg::DeviceStatus s = lfg::upload<lfg::HipDevice>(host, bytes, out);
    if (s.ok()) return LFG_OK;
    return fail_hip(ctx, (hipError_t)s.error, ((s.failed == lfg::DeviceStep::Allocate ? "hipMalloc(" : "hipMemcpy(") + std::string(what) + ")").c_str());
}

// The one place that evicts: at the top of an entry point, before its first lookup in `cache` (lfg_table_cache.hpp: TableCache).
template <class Cache>
void trim_tables(lfg_context *ctx, Cache &cache) {
    cache.trim([&] { (void)sync_lanes(ctx); });                 // a queued kernel may still read what goes
}

int build_axis_table(lfg_context *ctx, int in_size, int out_size, lfg::AxisTable *out) {
    if (const auto hit = ctx->tables.find(std::make_pair(in_size, out_size))) { *out = *hit; return LFG_OK; }

    std::vector<int> start((size_t)out_size);
    std::vector<float> weight((size_t)out_size * 6u);
    const float ts = 1.0f / (float)in_size;                    // scale.comp:23
    for (int p = 0; p < out_size; ++p) {
        const float uv = ((float)p + 0.5f) / (float)out_size;  // scale.comp:57
        const float pp = uv * (float)in_size - 0.5f;           // :24
        const float fl = std::floor(pp);
        const float f = pp - fl;                               // :25 fract
        const float s = fl - 2.0f;                             // :26
        double raw[6], sum = 0.0;
        for (int k = 0; k < 6; ++k) {
            const float sp = (s + (float)k + 0.5f) * ts;       // :33
            const bool skip = sp < 0.0f || sp > 1.0f;          // :34-37
            raw[k] = skip ? 0.0 : (double)lanczos_ref((float)k - f - 2.0f);   // :39-41
            sum += raw[k];
        }
        start[(size_t)p] = (int)s;
        for (int k = 0; k < 6; ++k) weight[(size_t)p * 6u + (size_t)k] = (float)(raw[k] / sum);   // :48
    }
    lfg::AxisTable t;
    t.in_size = in_size; t.out_size = out_size;
    t.pattern_2x = (out_size == 2 * in_size);
    if (t.pattern_2x)
        for (int k = 0; k < in_size; ++k)
            if (start[(size_t)(2 * k)] != k - 3 || start[(size_t)(2 * k + 1)] != k - 2) { t.pattern_2x = false; break; }

    // The distinct weight rows of a 2x table and each column's class (lfg_internal.hpp: AxisTable).
    std::vector<uint8_t> cls;
    std::vector<float> palette;
    if (t.pattern_2x) {
        cls.assign(((size_t)out_size + 3u) & ~(size_t)3u, 0);
        int rows = 0;
        for (int p = 0; p < out_size && rows >= 0; ++p) {
            const float *w = &weight[(size_t)p * 6u];
            int c = 0;
            while (c < rows && std::memcmp(&palette[(size_t)c * 8u], w, 6 * sizeof(float)) != 0) ++c;
            if (c == rows) {
                if (rows == 255) { rows = -1; break; }                       // not a palette any more: leave it out
                palette.insert(palette.end(), w, w + 6);
                palette.push_back(0.0f); palette.push_back(0.0f);
                ++rows;
            }
            cls[(size_t)p] = (uint8_t)c;
        }
        t.palette_rows = rows > 0 ? rows : 0;
    }

    if (t.pattern_2x) t.strips_per_xcd = lfg::scale_2x_strips_per_xcd(in_size);

    // start | weight | class | palette (the last two where there is a palette), each at a multiple of 256 bytes
    const auto up256 = [](size_t n) { return (n + 255u) & ~(size_t)255u; };
    const size_t offWeight = up256(start.size() * sizeof(int)), offClass = offWeight + up256(weight.size() * sizeof(float));
    const size_t offPalette = offClass + (t.palette_rows ? up256(cls.size()) : 0u);
    std::vector<uint8_t> host(offPalette + (t.palette_rows ? palette.size() * sizeof(float) : 0u), 0);
    memcpy(host.data(), start.data(), start.size() * sizeof(int));
    memcpy(host.data() + offWeight, weight.data(), weight.size() * sizeof(float));
    if (t.palette_rows) {
        memcpy(host.data() + offClass, cls.data(), cls.size());
        memcpy(host.data() + offPalette, palette.data(), palette.size() * sizeof(float));
    }
    const int rc = upload_table(ctx, host.data(), host.size(), "tables", &t.d_base);
    if (rc != LFG_OK) return rc;
    t.d_start = reinterpret_cast<int *>(t.d_base);
    t.d_weight = reinterpret_cast<float *>(t.d_base + offWeight);
    if (t.palette_rows) {
        t.d_class = t.d_base + offClass;
        t.d_palette = reinterpret_cast<float *>(t.d_base + offPalette);
    }
    ctx->tables.insert(t);
    *out = t;
    return LFG_OK;
}

// A frame the selected lane owns (mv_tmp, mv_refined, mv_bwd, mv_bwd_refined, half_prev, half_curr, mv_half, mvq_tmp, mid_tmp, levelled_prev), at this size: kept while the size stays, made again when it
// changes.  The test comes first because lfg_frame_destroy waits for every lane.  (frame_manager.cpp:226-230)
int lane_frame(lfg_context *ctx, lfg_frame &f, uint32_t width, uint32_t height, uint32_t format) {
    if (f.data && f.width == width && f.height == height) return LFG_OK;
    lfg_frame_destroy(ctx, &f);
    return lfg_frame_create(ctx, width, height, format, &f);
}

// The one place that grows a buffer of the selected lane (lfg_lane_state::buffers; lfg_table_cache.hpp: grow).  `what` names the
// allocation in the error.
int lane_buffer_grow(lfg_context *ctx, lfg::DeviceBuffer &buf, size_t need, const char *what) {
    const lfg::DeviceStatus s = lfg::grow<lfg::HipDevice>(buf, need, [&] { return (int)hipStreamSynchronize(ctx->cur().stream); });
    if (s.ok()) return LFG_OK;
    return fail_hip(ctx, (hipError_t)s.error, s.failed == lfg::DeviceStep::Synchronize ? "hipStreamSynchronize(cur.stream)" : what);
}

// uv table of one axis length (lfg_internal.hpp: UvTable); a handful of sizes per context.
int build_uv_table(lfg_context *ctx, int size, lfg::UvTable *out) {
    if (const auto hit = ctx->uv_tables.find(size)) { *out = *hit; return LFG_OK; }
    const size_t n4 = ((size_t)size + 3u) & ~(size_t)3u, quads = n4 / 4u;
    std::vector<float> uv(n4, 0.0f);
    std::vector<uint8_t> centre(n4, 0);
    for (int p = 0; p < size; ++p) {
        uv[(size_t)p] = ((float)p + 0.5f) / (float)size;                                  // interpolate.comp:30
        // texture() at uv[p] itself (csrc/lfg_interp.hpp: texture_bilinear, the same two roundings): texel p, fraction 0?
        const float u = uv[(size_t)p] * (float)size - 0.5f;
        const float fu = floorf(u);
        centre[(size_t)p] = (fu == (float)p && u - fu == 0.0f) ? 1 : 0;
    }
    lfg::UvTable t;
    t.size = size;
    t.blocks = (int)((quads + 63u) / 64u);
    std::vector<uint64_t> good((size_t)t.blocks, 0ull);
    for (size_t q = 0; q < quads; ++q)
        if (4 * q + 3 < (size_t)size && centre[4 * q] && centre[4 * q + 1] && centre[4 * q + 2] && centre[4 * q + 3])
            good[q / 64u] |= 1ull << (q % 64u);
    // the three-instruction uv of the kernels (lfg_internal.hpp: UvTable::rcp): exact for every p of this axis?
    t.rcp = 1.0f / (float)size;
    t.rcpExact = true;
    for (int p = 0; p < size && t.rcpExact; ++p) {
        const float x = (float)p + 0.5f, q0 = x * t.rcp;
        t.rcpExact = fmaf(fmaf(-q0, (float)size, x), t.rcp, q0) == uv[(size_t)p];
    }
    const size_t c64 = ((size_t)size + 63u) & ~(size_t)63u;
    const size_t offCentre = n4 * sizeof(float), offGood = (offCentre + c64 + 15u) & ~(size_t)15u;
    const size_t bytes = offGood + good.size() * sizeof(uint64_t) + 16u;
    std::vector<uint8_t> host(bytes, 0);
    memcpy(host.data(), uv.data(), n4 * sizeof(float));
    memcpy(host.data() + offCentre, centre.data(), n4);
    memcpy(host.data() + offGood, good.data(), good.size() * sizeof(uint64_t));
    const int rc = upload_table(ctx, host.data(), bytes, "uv table", &t.d_base);
    if (rc != LFG_OK) return rc;
    t.d_uv = reinterpret_cast<float *>(t.d_base);
    t.d_centre = t.d_base + offCentre;
    t.d_goodMask = reinterpret_cast<uint64_t *>(t.d_base + offGood);
    ctx->uv_tables.insert(t);
    *out = t;
    return LFG_OK;
}

// Both axes' tables of one interpolate call.
int interp_tables(lfg_context *ctx, int width, int height, lfg::InterpTables *tb) {
    trim_tables(ctx, ctx->uv_tables);
    lfg::UvTable tx, ty;
    int rc = build_uv_table(ctx, width, &tx);
    if (rc == LFG_OK) rc = build_uv_table(ctx, height, &ty);
    if (rc != LFG_OK) return rc;
    tb->uvx = tx.d_uv; tb->uvy = ty.d_uv;
    tb->centreX = tx.d_centre; tb->centreY = ty.d_centre;
    tb->goodMask = tx.d_goodMask;
    tb->rcpW = tx.rcp; tb->rcpH = ty.rcp; tb->rcpExact = tx.rcpExact && ty.rcpExact ? 1 : 0;
    return LFG_OK;
}

// ---- candidate tables of the 8/16 motion paths, both tie-break rules (tiny; built at the first lfg_motion)

int ensure_motion_tables(lfg_context *ctx) {
    if (ctx->motion_tables) return LFG_OK;
    std::vector<uint32_t> host(7 * lfg::kMotionTableWords, 0u);
    for (int sem = 0; sem < 2; ++sem)
        lfg::motion_tables(sem != 0, host.data() + (3 * sem) * lfg::kMotionTableWords,
                           host.data() + (3 * sem + 1) * lfg::kMotionTableWords,
                           host.data() + (3 * sem + 2) * lfg::kMotionTableWords, host.data() + 6 * lfg::kMotionTableWords);
    // Published only once the copy has succeeded: a later call must never find a half-initialised table.
    uint8_t *d = nullptr;
    const int rc = upload_table(ctx, host.data(), host.size() * sizeof(uint32_t), "motion tables", &d);
    if (rc == LFG_OK) ctx->motion_tables = reinterpret_cast<uint32_t *>(d);
    return rc;
}

// ---- scratch of the prefiltered motion path (per frame size; kept between calls)

// Parts of the candidate order per rim segment (motion_plan.hip: prefilter_plan), measured at 4K (frames/s):
//   4   the default with frames in flight (lfg_lanes >= 2), where the sum of all units' times is what counts: pan 2,838;
//   48  four, and eight for the segments whose position rows leave the image at its top or bottom -- the strip a vertical pan
//       exposes is the longest unit of a frame, and the launch is as long as its longest unit when ONE frame runs at a time:
//       the default there.  One frame at a time: pan 1,868 -> 2,307 (motion 0.49 -> 0.38 ms), noisy 889 -> 981, stills
//       3,880 -> 3,976, occluded 815 -> 810, moving objects 976 -> 971; with three frames in flight it costs 1 - 2 %
//       (134 more workgroups that stage a window each), which is why it is not used there;
//   8   every rim segment in eight parts: one frame at a time the pan gains less (2,050) and everything else loses 5 - 10 %;
//       9 % slower with three frames in flight.
// LFG_MOTION_RIM_SPLIT=4|8|48 overrides (read ONCE, when the context is created).  The plan therefore changes only where the lane
// count does -- inside lfg_lanes(), never silently between two lfg_motion calls -- and lfg_motion_plan() reports it.
int motion_rim_split(const lfg_context *ctx) {
    if (ctx->rim_split_env) return ctx->rim_split_env;
    return ctx->lanes.size() >= 2 ? 4 : 48;
}
// Round 4: with frames in flight a call whose content suits it -- the order kernel's verdict on the lane's previous call -- sends
// its whole interior tiles through the lean kernel first (motion_lean.hip).  What is left to the persistent kernel then is the
// rim, its longest units set the launch's length again, and 48 wins there as well (pan 3,250 -> 3,345 frames/s with three
// frames in flight; noise -5 %, stills -4 %: which is why it is this plan only for those calls).  Both plans are resident.
int motion_rim_split_lean(const lfg_context *ctx) {
    return (ctx->motion_lean && ctx->lanes.size() >= 2 && !ctx->rim_split_env) ? 48 : 0;
}

int ensure_motion_workspace(lfg_context *ctx, uint32_t width, uint32_t height) {
    lfg_lane_state &cur = ctx->cur();
    const int rimSplit = motion_rim_split(ctx), rimSplit2 = motion_rim_split_lean(ctx);
    if (cur.motion_ws.data && cur.motion_ws_w == width && cur.motion_ws_h == height && cur.motion_ws_layout.rimSplit == rimSplit &&
        cur.motion_ws_layout.rimSplit2 == rimSplit2) return LFG_OK;
    lfg::MotionWorkspaceLayout layout;
    if (ctx->motion_slots == 0) {
        ctx->motion_slots = lfg::prefilter_slots();
        if (ctx->knobs.debug) fprintf(stderr, "lfg: motion prefilter: %d workgroups resident at once\n", ctx->motion_slots);
    }
    const size_t bytes = lfg::motion_workspace_bytes(width, height, ctx->motion_slots, rimSplit, rimSplit2, &layout);
    if (bytes > cur.motion_ws.bytes) {
        const int rc = lane_buffer_grow(ctx, cur.motion_ws, bytes, "hipMalloc((void **)&cur.motion_ws, bytes)");
        if (rc != LFG_OK) return rc;
    } else {
        LFG_HIP(ctx, hipStreamSynchronize(cur.stream));          // a queued kernel may still read the plan tables about to be overwritten
    }
    // work-unit tables of this frame size: unitMap | unitAux | tileMap
    const lfg::PrefilterPlanHost plan = lfg::prefilter_plan(width, height, ctx->motion_slots, rimSplit);
    std::vector<uint32_t> tables;
    tables.insert(tables.end(), plan.unitMap.begin(), plan.unitMap.end());
    tables.insert(tables.end(), plan.unitAux.begin(), plan.unitAux.end());
    tables.insert(tables.end(), plan.tileMap.begin(), plan.tileMap.end());
    LFG_HIP(ctx, hipMemcpy(cur.motion_ws.data + layout.plan, tables.data(), tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (rimSplit2) {        // the plan of the calls that go through the lean kernel, and that kernel's tiles
        const lfg::PrefilterPlanHost plan2 = lfg::prefilter_plan(width, height, ctx->motion_slots, rimSplit2);
        std::vector<uint32_t> t2;
        t2.insert(t2.end(), plan2.unitMap.begin(), plan2.unitMap.end());
        t2.insert(t2.end(), plan2.unitAux.begin(), plan2.unitAux.end());
        t2.insert(t2.end(), plan2.tileMap.begin(), plan2.tileMap.end());
        LFG_HIP(ctx, hipMemcpy(cur.motion_ws.data + layout.plan2, t2.data(), t2.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (!plan2.leanTiles.empty()) {
            std::vector<uint32_t> listed = plan2.leanTiles;
            listed.insert(listed.end(), plan2.leanPartial.begin(), plan2.leanPartial.end());
            LFG_HIP(ctx, hipMemcpy(cur.motion_ws.data + layout.leanTiles, listed.data(), listed.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    // what the kernels expect to find between calls: a cleared control area (the hint kernel's counter of finished
    // workgroups lies in it, and that kernel is what clears the rest per call) and the merge words of the flagged tiles all ones
    LFG_HIP(ctx, hipMemset(cur.motion_ws.data + layout.tileFlags, 0, layout.order - layout.tileFlags));
    LFG_HIP(ctx, hipMemset(cur.motion_ws.data + layout.merge, 0xFF, layout.mergeBytes));
    cur.motion_units = plan.units;
    layout.lastLean = 0;
    cur.motion_ws_layout = layout;
    cur.motion_ws_w = width; cur.motion_ws_h = height;
    return LFG_OK;
}

// ---- profiling

struct StageTimer {
    lfg_context *ctx;
    hipEvent_t b = nullptr, e = nullptr;
    int stage;
    StageTimer(lfg_context *c, int st) : ctx(c), stage(st) {
        if (!ctx->profile) return;
        if (!ctx->prof_free.empty()) { b = ctx->prof_free.back().first; e = ctx->prof_free.back().second; ctx->prof_free.pop_back(); }
        else if (hipEventCreate(&b) != hipSuccess || hipEventCreate(&e) != hipSuccess) { b = e = nullptr; return; }
        (void)hipEventRecord(b, ctx->cur().stream);
    }
    ~StageTimer() {
        if (!b) return;
        (void)hipEventRecord(e, ctx->cur().stream);
        lfg::ProfileSlot s; s.begin = b; s.end = e; s.stage = stage;
        ctx->prof_pending.push_back(s);
    }
};

int drain_profile(lfg_context *ctx) {
    if (ctx->prof_pending.empty()) return LFG_OK;
    LFG_HIP(ctx, sync_lanes(ctx));
    for (auto &s : ctx->prof_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.begin, s.end) == hipSuccess) { ctx->prof_ms[s.stage] += ms; ctx->prof_n[s.stage] += 1; }
        ctx->prof_free.emplace_back(s.begin, s.end);
    }
    ctx->prof_pending.clear();
    return LFG_OK;
}

}  // namespace

struct lfg_ring {
    lfg_context *ctx = nullptr;
    uint32_t slots = 0;
    size_t slot_bytes = 0;
    uint8_t *base = nullptr;                 // pinned host memory, slots * slot_bytes
    std::vector<hipEvent_t> done;            // last transfer touching each slot
    std::vector<uint8_t> busy;
    uint32_t next = 0;
    hipStream_t copy = nullptr;              // transfers run here, next to the kernels on the selected lane's stream
    hipEvent_t ready = nullptr;              // scratch event: "the selected lane's stream has reached this point"
};

// ================================================================== library / context

// A stream of the library's own.  While a communicator exists (ctx->comm_cus > 0, lfg_comm.cpp) it carries a CU mask that leaves
// the first comm_cus CUs to the communication stream, which is masked to exactly those: RCCL's device kernel needs CUs without a
// persistent prefilter workgroup on them (comm_probe.hip), and only the pair of masks guarantees it gets them (lfg_comm_init).  Mask bit i is CU i / 8 of XCD i % 8 on an MI355X (tools/probe_cu_mask.hip
// on the device: clearing bits 0 - 7 takes one CU out of each of the eight XCDs), so 8 | 16 | 24 | 32 bits are 1 - 4 CUs per XCD, where
// the hardware's round-robin of workgroups over the XCDs puts the communicator's 8 - 32 channels.
// (A stream made by hipExtStreamCreateWithCUMask has default flags: it synchronises with the NULL stream, which the library never uses.)
hipError_t lfg_own_stream_create(const lfg_context *ctx, hipStream_t *out) {
    if (!ctx || ctx->comm_cus <= 0) return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    if (e != hipSuccess) return e;
    if (cus <= ctx->comm_cus) return hipErrorInvalidValue;
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0xffffffffu);
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
    for (int i = 0; i < ctx->comm_cus; ++i) mask[(size_t)i / 32] &= ~(1u << (i % 32));
    return hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data());
}

// Every stream the library owns is made again under the current reservation (the communicator has just come or gone).  A stream the
// caller supplied (lfg_context_set_stream) is the caller's to mask: lfg_comm_cu_mask says how.
int lfg_restream(lfg_context *ctx) {
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    auto again = [&](hipStream_t &own, hipStream_t &used) -> hipError_t {
        if (!own) return hipSuccess;
        hipError_t e = hipStreamSynchronize(own);
        hipStream_t fresh = nullptr;
        if (e == hipSuccess) e = lfg_own_stream_create(ctx, &fresh);
        if (e != hipSuccess) return e;
        (void)hipStreamDestroy(own);
        if (used == own) used = fresh;
        own = fresh;
        return hipSuccess;
    };
    for (size_t k = 0; k < ctx->lanes.size(); ++k) {
        lfg_lane_state &l = ctx->from_selected(k);
        LFG_HIP(ctx, again(l.own_stream, l.stream));
    }
    return LFG_OK;
}

LFG_EXPORT int lfg_abi_version(void) { return LFG_ABI_VERSION; }

LFG_EXPORT int lfg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

LFG_EXPORT int lfg_context_create(int device_ordinal, lfg_context **out_ctx) {
    if (!out_ctx) return fail(nullptr, LFG_ERR_INVALID, "lfg_context_create: out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, LFG_ERR_DEVICE, std::string("lfg_context_create: no HIP device (") +
                                                 (e != hipSuccess ? hipGetErrorString(e) : "count 0") + "); there is no CPU fallback");
    const int dev = device_ordinal < 0 ? 0 : device_ordinal;
    if (dev >= n) return fail(nullptr, LFG_ERR_INVALID, "lfg_context_create: device ordinal out of range");
    LFG_HIP(nullptr, hipSetDevice(dev));
    lfg_context *ctx = new (std::nothrow) lfg_context();
    if (!ctx) return fail(nullptr, LFG_ERR_NOMEM, "lfg_context_create: out of host memory");
    ctx->device = dev;
    (void)hipDeviceGetAttribute(&ctx->device_cus, hipDeviceAttributeMultiprocessorCount, dev);
    lfg_lane_state lane0;
    e = lfg_own_stream_create(ctx, &lane0.own_stream);
    if (e != hipSuccess) { delete ctx; return fail_hip(nullptr, e, "hipStreamCreate"); }
    lane0.stream = lane0.own_stream;
    ctx->lanes.push_back(lane0);
    if (const char *m = getenv("LFG_MOTION_HINTS")) ctx->motion_hints = atoi(m) != 0;
    if (const char *m = getenv("LFG_MOTION_LEAN")) ctx->motion_lean = atoi(m) != 0;
    if (const char *m = getenv("LFG_MOTION_RIM_SPLIT")) { const int v = atoi(m); if (v == 4 || v == 8 || v == 48) ctx->rim_split_env = v; }
    if (const char *m = getenv("LFG_FUSED_INTERPOLATE_SCALE")) ctx->fuse_interpolate_scale = atoi(m) != 0;
    if (const char *m = getenv("LFG_FUSED_MOTION_INTERPOLATE")) ctx->fuse_motion_interpolate = atoi(m) != 0;
    if (const char *m = getenv("LFG_MOTION_MODE")) ctx->motion_mode = atoi(m) == 1 ? LFG_MOTION_EXACT_ONLY : LFG_MOTION_PREFILTERED;
    // measurement knobs (lfg_internal.hpp: MotionKnobs): here and nowhere else -- no call reads the environment
    if (const char *m = getenv("LFG_LEAN_FORCE")) ctx->knobs.leanForce = atoi(m) & 1;
    if (getenv("LFG_FALLBACK_FULL")) ctx->knobs.fallbackFull = 1;
    if (const char *m = getenv("LFG_DYN_PARTS_RT")) ctx->knobs.dynParts = atoi(m);
    if (const char *m = getenv("LFG_PREF_GROUPS")) ctx->knobs.prefGroups = atoi(m);
    if (const char *m = getenv("LFG_RESOLVE_GROUPS")) ctx->knobs.resolveGroups = atoi(m);
    if (const char *m = getenv("LFG_MOTION_STRIP")) ctx->knobs.strips = atoi(m) != 0;
    if (const char *m = getenv("LFG_STRIP_PAD")) ctx->knobs.stripPad = atoi(m);
    if (getenv("LFG_DEBUG")) ctx->knobs.debug = 1;
    if (getenv("LFG_DEBUG_DYN")) ctx->knobs.debugDyn = 1;
    if (const char *m = getenv("LFG_DEBUG_DYN_DEEP")) ctx->knobs.debugDynDeep = atoi(m);
    if (const char *m = getenv("LFG_TIER_FORCE")) ctx->knobs.tierForce = atoi(m) & 1;
    if (const char *m = getenv("LFG_FILL_BAND")) { const int v = atoi(m); if (v >= 8 && v <= 1024) ctx->knobs.fillBand = v; }
    if (const char *m = getenv("LFG_COMM_CUS")) { const int v = atoi(m); if (v == 0 || v == 8 || v == 16 || v == 24 || v == 32) ctx->knobs.commCus = v; }
    *out_ctx = ctx;
    return LFG_OK;
}

namespace {
void lane_release(lfg_lane_state &l) {
    if (l.stream) (void)hipStreamSynchronize(l.stream);
    if (l.own_stream && l.own_stream != l.stream) (void)hipStreamSynchronize(l.own_stream);
    for (lfg_frame *f : {&l.mv_tmp, &l.mv_refined, &l.mv_bwd, &l.mv_bwd_refined, &l.half_prev, &l.half_curr, &l.mv_half, &l.mvq_tmp, &l.mid_tmp, &l.levelled_prev})      // (lane_frame)
        if (f->data && f->owned) (void)hipFree(f->data);
    for (lfg::DeviceBuffer *b : l.buffers()) lfg::release<lfg::HipDevice>(*b);
    if (l.mark) (void)hipEventDestroy(l.mark);
    if (l.verdict.event) (void)hipEventDestroy(l.verdict.event);
    if (l.verdict.pinned) (void)hipHostFree(l.verdict.pinned);
    if (l.cut.event) (void)hipEventDestroy(l.cut.event);
    if (l.cut.pinned) (void)hipHostFree(l.cut.pinned);
    if (l.cut.device) (void)hipFree(l.cut.device);
    if (l.levels.event) (void)hipEventDestroy(l.levels.event);
    if (l.levels.pinned) (void)hipHostFree(l.levels.pinned);
    if (l.levels.device) (void)hipFree(l.levels.device);
    if (l.own_stream) (void)hipStreamDestroy(l.own_stream);
    l = lfg_lane_state{};
}
}  // namespace

LFG_EXPORT void lfg_context_destroy(lfg_context *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)lfg_comm_destroy(ctx);
    (void)sync_lanes(ctx);
    for (auto &l : ctx->lanes) lane_release(l);
    for (auto &s : ctx->prof_pending) { (void)hipEventDestroy(s.begin); (void)hipEventDestroy(s.end); }
    for (auto &p : ctx->prof_free) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    ctx->tables.release_all(); ctx->uv_tables.release_all(); ctx->resample_tables.release_all();
    ctx->resample_brackets.release_all(); ctx->edge_positions.release_all();
    if (ctx->edge_shapes) (void)hipFree(ctx->edge_shapes);
    for (uint32_t *t : ctx->light_tables) if (t) (void)hipFree(t);
    if (ctx->motion_tables) (void)hipFree(ctx->motion_tables);
    delete ctx;
}

LFG_EXPORT int lfg_context_set_stream(lfg_context *ctx, void *hip_stream) {
    if (!ctx) return LFG_ERR_INVALID;
    int rc = drain_profile(ctx);
    if (rc != LFG_OK) return rc;
    LFG_HIP(ctx, hipStreamSynchronize(ctx->cur().stream));
    ctx->cur().stream = hip_stream ? (hipStream_t)hip_stream : ctx->cur().own_stream;
    return LFG_OK;
}

LFG_EXPORT void *lfg_context_get_stream(lfg_context *ctx) { return ctx ? (void *)ctx->cur().stream : nullptr; }

// ------------------------------------------------------------------ lanes: several frames in flight on one GPU

LFG_EXPORT int lfg_lanes(lfg_context *ctx, int count) {
    if (!ctx) return LFG_ERR_INVALID;
    if (count < 1 || count > LFG_MAX_LANES) return fail(ctx, LFG_ERR_INVALID, "lfg_lanes: count must be 1 .. LFG_MAX_LANES");
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->lane >= count) ctx->lane = 0;     // the selected lane is about to go: back to lane 0 first
    while ((int)ctx->lanes.size() > count) { lane_release(ctx->lanes.back()); ctx->lanes.pop_back(); }
    while ((int)ctx->lanes.size() < count) {
        lfg_lane_state l;
        hipError_t e = lfg_own_stream_create(ctx, &l.own_stream);
        if (e != hipSuccess) return fail_hip(ctx, e, "hipStreamCreate (lane)");
        l.stream = l.own_stream;
        ctx->lanes.push_back(l);
    }
    return LFG_OK;
}

LFG_EXPORT int lfg_lane_count(const lfg_context *ctx) { return ctx ? (int)ctx->lanes.size() : 0; }
LFG_EXPORT int lfg_lane_current(const lfg_context *ctx) { return ctx ? ctx->lane : -1; }

LFG_EXPORT int lfg_lane_select(lfg_context *ctx, int lane) {
    if (!ctx) return LFG_ERR_INVALID;
    if (lane < 0 || lane >= (int)ctx->lanes.size()) return fail(ctx, LFG_ERR_INVALID, "lfg_lane_select: no such lane (lfg_lanes first)");
    ctx->lane = lane;
    return LFG_OK;
}

LFG_EXPORT int lfg_lane_mark(lfg_context *ctx) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->cur().mark) LFG_HIP(ctx, hipEventCreateWithFlags(&ctx->cur().mark, hipEventDisableTiming));
    LFG_HIP(ctx, hipEventRecord(ctx->cur().mark, ctx->cur().stream));
    ctx->cur().marked = true;
    return LFG_OK;
}

LFG_EXPORT int lfg_lane_wait(lfg_context *ctx, int other) {
    if (!ctx) return LFG_ERR_INVALID;
    if (other < 0 || other >= (int)ctx->lanes.size()) return fail(ctx, LFG_ERR_INVALID, "lfg_lane_wait: no such lane");
    if (other == ctx->lane) return LFG_OK;     // a stream is in order with itself
    const lfg_lane_state &o = ctx->lanes[(size_t)other];
    if (!o.marked) return LFG_OK;              // nothing to wait for yet
    LFG_HIP(ctx, hipStreamWaitEvent(ctx->cur().stream, o.mark, 0));
    return LFG_OK;
}

LFG_EXPORT int lfg_lane_sync(lfg_context *ctx) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    LFG_HIP(ctx, hipStreamSynchronize(ctx->cur().stream));
    return LFG_OK;
}

LFG_EXPORT int lfg_context_device(const lfg_context *ctx) { return ctx ? ctx->device : -1; }

LFG_EXPORT int lfg_sync(lfg_context *ctx) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, sync_lanes(ctx));             // every lane: "the device is idle" is what callers mean
    return LFG_OK;
}

LFG_EXPORT const char *lfg_last_error(const lfg_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

// ================================================================== frames

LFG_EXPORT int lfg_frame_create(lfg_context *ctx, uint32_t width, uint32_t height, uint32_t format, lfg_frame *out) {
    if (!ctx || !out) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_create: NULL argument");
    const uint32_t bpp = bytes_per_pixel(format);
    if (!bpp || width == 0 || height == 0 || width > 32768u || height > 32768u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_create: bad size or format");
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    void *p = nullptr;
    const size_t bytes = (size_t)width * (size_t)height * (size_t)bpp;
    LFG_HIP(ctx, hipMalloc(&p, bytes));
    out->data = p; out->width = width; out->height = height; out->pitch = width * bpp;
    out->format = format; out->owned = 1; out->reserved = 0;
    return LFG_OK;
}

LFG_EXPORT void lfg_frame_destroy(lfg_context *ctx, lfg_frame *frame) {
    if (!frame) return;
    if (frame->data && frame->owned) {
        if (ctx) { (void)hipSetDevice(ctx->device); (void)sync_lanes(ctx); }
        (void)hipFree(frame->data);
    }
    frame->data = nullptr; frame->width = frame->height = frame->pitch = 0; frame->owned = 0;
}

LFG_EXPORT int lfg_frame_wrap(void *device_ptr, uint32_t width, uint32_t height, uint32_t pitch, uint32_t format,
                              lfg_frame *out) {
    const uint32_t bpp = bytes_per_pixel(format);
    if (!out || !device_ptr || !bpp || width == 0 || height == 0 || pitch > kMaxFramePitch ||
        (uint64_t)pitch < (uint64_t)width * bpp)
        return LFG_ERR_INVALID;
    out->data = device_ptr; out->width = width; out->height = height; out->pitch = pitch;
    out->format = format; out->owned = 0; out->reserved = 0;
    return LFG_OK;
}

LFG_EXPORT int lfg_frame_copy(lfg_context *ctx, const lfg_frame *src, lfg_frame *dst) {
    if (!ctx || !src || !dst || !src->data || !dst->data) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_copy: NULL frame");
    if (pitch_too_large(src) || pitch_too_large(dst)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_copy: a pitch above 0x7fffffff");
    if (!same_size(src, dst) || src->format != dst->format)                  // frame_manager.cpp:84-87
        return fail(ctx, LFG_ERR_INVALID, "Source and destination frame dimensions do not match");
    const size_t row = (size_t)src->width * bytes_per_pixel(src->format);
    LFG_HIP(ctx, hipMemcpy2DAsync(dst->data, dst->pitch, src->data, src->pitch, row, src->height,
                                  hipMemcpyDeviceToDevice, ctx->cur().stream));
    return LFG_OK;
}

LFG_EXPORT int lfg_staging_create(lfg_context *ctx, size_t bytes, void **out_host_ptr) {
    if (!ctx || !out_host_ptr || bytes == 0) return fail(ctx, LFG_ERR_INVALID, "lfg_staging_create: bad argument");
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    LFG_HIP(ctx, hipHostMalloc(out_host_ptr, bytes, hipHostMallocDefault));
    return LFG_OK;
}

LFG_EXPORT void lfg_staging_destroy(lfg_context *ctx, void *host_ptr) {
    if (!host_ptr) return;
    if (ctx) (void)sync_lanes(ctx);
    (void)hipHostFree(host_ptr);
}

LFG_EXPORT int lfg_frame_upload(lfg_context *ctx, lfg_frame *dst, const void *host, size_t bytes) {
    if (!ctx || !dst || !dst->data || !host) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_upload: NULL argument");
    if (pitch_too_large(dst)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_upload: a pitch above 0x7fffffff");
    const size_t row = (size_t)dst->width * bytes_per_pixel(dst->format);
    if (bytes < row * dst->height) {                                          // window_capture.cpp:478-481
        char msg[160];
        snprintf(msg, sizeof msg, "Captured image size (%zu) smaller than expected (%zu)", bytes, row * dst->height);
        return fail(ctx, LFG_ERR_INVALID, msg);
    }
    LFG_HIP(ctx, hipMemcpy2DAsync(dst->data, dst->pitch, host, row, row, dst->height, hipMemcpyHostToDevice, ctx->cur().stream));
    return LFG_OK;
}

LFG_EXPORT int lfg_frame_download(lfg_context *ctx, const lfg_frame *src, void *host, size_t bytes) {
    if (!ctx || !src || !src->data || !host) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_download: NULL argument");
    if (pitch_too_large(src)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_download: a pitch above 0x7fffffff");
    const size_t row = (size_t)src->width * bytes_per_pixel(src->format);
    if (bytes < row * src->height) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_download: host buffer too small");
    LFG_HIP(ctx, hipMemcpy2DAsync(host, row, src->data, src->pitch, row, src->height, hipMemcpyDeviceToHost, ctx->cur().stream));
    return LFG_OK;
}

// ================================================================== pinned-host frame ring

LFG_EXPORT int lfg_ring_create(lfg_context *ctx, uint32_t slots, size_t slot_bytes, lfg_ring **out_ring) {
    if (!ctx || !out_ring || slots == 0 || slots > 64 || slot_bytes == 0)
        return fail(ctx, LFG_ERR_INVALID, "lfg_ring_create: bad argument");
    lfg_ring *r = new (std::nothrow) lfg_ring();
    if (!r) return fail(ctx, LFG_ERR_NOMEM, "lfg_ring_create: out of host memory");
    r->ctx = ctx; r->slots = slots; r->slot_bytes = (slot_bytes + 4095u) & ~(size_t)4095u;
    hipError_t e = hipHostMalloc((void **)&r->base, r->slot_bytes * slots, hipHostMallocDefault);
    if (e != hipSuccess) { delete r; return fail_hip(ctx, e, "hipHostMalloc(ring)"); }
    r->done.resize(slots, nullptr); r->busy.assign(slots, 0);
    e = hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ready, hipEventDisableTiming);
    if (e != hipSuccess) { lfg_ring_destroy(r); return fail_hip(ctx, e, "hipStreamCreate(ring)"); }
    for (uint32_t i = 0; i < slots; ++i) {
        e = hipEventCreateWithFlags(&r->done[i], hipEventDisableTiming);
        if (e != hipSuccess) { lfg_ring_destroy(r); return fail_hip(ctx, e, "hipEventCreate(ring)"); }
    }
    *out_ring = r;
    return LFG_OK;
}

LFG_EXPORT void lfg_ring_destroy(lfg_ring *ring) {
    if (!ring) return;
    if (ring->copy) (void)hipStreamSynchronize(ring->copy);
    for (uint32_t i = 0; i < ring->slots; ++i)
        if (ring->done[i]) { if (ring->busy[i]) (void)hipEventSynchronize(ring->done[i]); (void)hipEventDestroy(ring->done[i]); }
    if (ring->ready) (void)hipEventDestroy(ring->ready);
    if (ring->copy) (void)hipStreamDestroy(ring->copy);
    if (ring->base) (void)hipHostFree(ring->base);
    delete ring;
}

LFG_EXPORT int lfg_ring_acquire(lfg_ring *ring, void **out_host_ptr, uint32_t *out_slot) {
    if (!ring || !out_host_ptr || !out_slot) return LFG_ERR_INVALID;
    const uint32_t s = ring->next;
    ring->next = (ring->next + 1) % ring->slots;
    if (ring->busy[s]) { LFG_HIP(ring->ctx, hipEventSynchronize(ring->done[s])); ring->busy[s] = 0; }
    *out_host_ptr = ring->base + (size_t)s * ring->slot_bytes;
    *out_slot = s;
    return LFG_OK;
}

// Transfers run on the ring's own stream so they overlap the kernels:
//   upload    copy stream waits for what the selected lane's stream has been given so far (earlier readers of `dst`),
//             copies, and that stream then waits for the copy -- kernels enqueued next see the pixels;
//   download  copy stream waits for what the selected lane's stream has been given so far (the producers of `src`) and copies;
//             that stream does NOT wait: before a kernel overwrites `src` again, call lfg_ring_fence_slot.
static int ring_transfer(lfg_ring *ring, uint32_t slot, const lfg_frame *f, bool upload) {
    lfg_context *ctx = ring->ctx;
    if (!f || !f->data) return fail(ctx, LFG_ERR_INVALID, "lfg_ring transfer: NULL frame");
    if (pitch_too_large(f)) return fail(ctx, LFG_ERR_INVALID, "lfg_ring transfer: a pitch above 0x7fffffff");
    const size_t row = (size_t)f->width * bytes_per_pixel(f->format), need = row * f->height;
    if (ring->slot_bytes < need) return fail(ctx, LFG_ERR_INVALID, "lfg_ring transfer: slot smaller than the frame");
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    uint8_t *host = ring->base + (size_t)slot * ring->slot_bytes;
    LFG_HIP(ctx, hipEventRecord(ring->ready, ctx->cur().stream));
    LFG_HIP(ctx, hipStreamWaitEvent(ring->copy, ring->ready, 0));
    if (upload) LFG_HIP(ctx, hipMemcpy2DAsync(f->data, f->pitch, host, row, row, f->height, hipMemcpyHostToDevice, ring->copy));
    else LFG_HIP(ctx, hipMemcpy2DAsync(host, row, f->data, f->pitch, row, f->height, hipMemcpyDeviceToHost, ring->copy));
    LFG_HIP(ctx, hipEventRecord(ring->done[slot], ring->copy));
    ring->busy[slot] = 1;
    if (upload) LFG_HIP(ctx, hipStreamWaitEvent(ctx->cur().stream, ring->done[slot], 0));
    return LFG_OK;
}

LFG_EXPORT int lfg_ring_upload(lfg_ring *ring, uint32_t slot, lfg_frame *dst) {
    if (!ring || slot >= ring->slots) return LFG_ERR_INVALID;
    return ring_transfer(ring, slot, dst, true);
}

LFG_EXPORT int lfg_ring_download(lfg_ring *ring, uint32_t slot, const lfg_frame *src) {
    if (!ring || slot >= ring->slots) return LFG_ERR_INVALID;
    return ring_transfer(ring, slot, src, false);
}

LFG_EXPORT int lfg_ring_wait(lfg_ring *ring, uint32_t slot) {
    if (!ring || slot >= ring->slots) return LFG_ERR_INVALID;
    if (ring->busy[slot]) { LFG_HIP(ring->ctx, hipEventSynchronize(ring->done[slot])); ring->busy[slot] = 0; }
    return LFG_OK;
}

LFG_EXPORT int lfg_ring_fence_slot(lfg_ring *ring, uint32_t slot) {
    if (!ring || slot >= ring->slots) return LFG_ERR_INVALID;
    if (ring->busy[slot]) LFG_HIP(ring->ctx, hipStreamWaitEvent(ring->ctx->cur().stream, ring->done[slot], 0));
    return LFG_OK;
}

// ================================================================== stages

LFG_EXPORT int lfg_scale(lfg_context *ctx, const lfg_frame *in, lfg_frame *out) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));          // the stream belongs to this device (multi-GPU hosts)
    if (!frame_ok(in, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_scale: frames must be non-empty RGBA8");
    if (in->data == out->data) return fail(ctx, LFG_ERR_INVALID, "lfg_scale: in-place scaling is not supported");
    trim_tables(ctx, ctx->tables);
    lfg::AxisTable tx, ty;
    int rc = build_axis_table(ctx, (int)in->width, (int)out->width, &tx);
    if (rc != LFG_OK) return rc;
    rc = build_axis_table(ctx, (int)in->height, (int)out->height, &ty);
    if (rc != LFG_OK) return rc;
    const bool fast = tx.pattern_2x && ty.pattern_2x && tx.palette_rows > 0 && ty.strips_per_xcd > 0 && lfg::scale_2x_supported(*in, *out);
    StageTimer timer(ctx, LFG_STAGE_SCALE);
    hipError_t e = fast ? lfg::launch_scale_2x(ctx->cur().stream, *in, *out, tx, ty)
                        : lfg::launch_scale_generic(ctx->cur().stream, *in, *out, tx, ty);
    if (e != hipSuccess) return fail_hip(ctx, e, "scale kernel launch");
    ctx->scale_last_kernel = fast ? 1 : 0;
    return LFG_OK;
}

LFG_EXPORT int lfg_scale_last_kernel(const lfg_context *ctx) { return ctx ? ctx->scale_last_kernel : -1; }

// lfg_motion, and -- fused != nullptr -- the motion stage of lfg_interpolate_frames in the north-star order: the kernels
// write the generated frame themselves (lfg_internal.hpp: FusedOut).  *fusedDone tells the caller whether they did (the
// generic kernel, for other block sizes, radii and frames of 2 GiB, does not).
static int motion_run(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *mv,
                      int block_size, float search_radius, const lfg::FusedOut *fused, bool *fusedDone) {
    if (fusedDone) *fusedDone = false;
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));          // the stream belongs to this device (multi-GPU hosts)
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) ||
        !frame_ok(mv, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion: prev/curr must be RGBA8 and mv MV_S8X2, all non-empty");
    if (!same_size(prev, curr) || !same_size(curr, mv))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion: prev, curr and mv differ in size");
    if (block_size < 1 || block_size > 64) return fail(ctx, LFG_ERR_UNSUPPORTED, "lfg_motion: blockSize must be in [1,64]");
    if (!(search_radius >= 0.0f) || search_radius > 127.0f || search_radius != std::floor(search_radius))
        return fail(ctx, LFG_ERR_UNSUPPORTED, "lfg_motion: searchRadius must be a whole number in [0,127]");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion: RGBA8 frames must be 4-byte aligned");
    const int R = (int)search_radius;
    // The 8/16 kernels address rows with 32-bit byte offsets and lean on the buffer range check for rows outside
    // the image ("negative" offsets wrap to >= 2^31): both hold only below 2 GiB per frame.  Larger frames take the
    // generic kernel, which indexes with size_t.
    const bool fits32 = (uint64_t)prev->height * prev->pitch < 0x7fffffffull && (uint64_t)curr->height * curr->pitch < 0x7fffffffull &&
                        (uint64_t)mv->height * mv->pitch < 0x7fffffffull;
    const bool tiled = block_size == 8 && R == 16 && fits32;
    const uint32_t *rank2scan = nullptr, *order32 = nullptr;
    if (tiled) {
        int rc = ensure_motion_tables(ctx);
        if (rc != LFG_OK) return rc;
        rank2scan = ctx->motion_tables + (3 * ctx->semantics) * lfg::kMotionTableWords;
        order32 = rank2scan + lfg::kMotionTableWords;
    }
    if (tiled && ctx->motion_mode == LFG_MOTION_PREFILTERED) {
        int rc = ensure_motion_workspace(ctx, curr->width, curr->height);
        if (rc != LFG_OK) return rc;
    }
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e;
    const lfg::FusedOut fo = (fused && tiled) ? *fused : lfg::FusedOut();
    if (tiled && ctx->motion_mode == LFG_MOTION_PREFILTERED) {
        // The lean kernel, the persistent grid, its variant and the second pass's grid are decided by the verdict of the lane's last
        // finished call (lfg_motion_verdict.hpp: motion_call_policy); here only what it takes from HIP.  The lean kernel's plan exists
        // with frames in flight only (one frame at a time it sits in front of the rim's long units: 2,620 -> 2,360 frames/s), and
        // serves either tie order (round 5: the intended order's ranks go through rank2scan).
        lfg_lane_state &cur = ctx->cur();
        lfg::MotionVerdictState &v = cur.verdict;
        if (lfg::motion_verdict_wanted((int)ctx->lanes.size(), ctx->motion_hints) && !v.pinned) {
            LFG_HIP(ctx, hipHostMalloc((void **)&v.pinned, sizeof(uint32_t), hipHostMallocDefault));
            *v.pinned = 0u;
            LFG_HIP(ctx, hipEventCreateWithFlags(&v.event, hipEventDisableTiming));
        }
        if (v.pending && hipEventQuery(v.event) == hipSuccess) {
            v.word = *v.pinned; v.pending = false; v.seen = true;
            const lfg::MotionVerdictScore score = lfg::motion_verdict_score(v.launchedOn, v.word);      // (lfg_motion_prediction_stats)
            ctx->pred_verdicts += 1;
            ctx->pred_lean_wrong += score.leanWrong;
            ctx->pred_grid_wrong += score.gridWrong;
            ctx->pred_second_wrong += score.secondWrong;
        }
        lfg::MotionCallInputs in;
        in.lanes = (int)ctx->lanes.size();
        in.hints = ctx->motion_hints;
        in.leanPlan = cur.motion_ws_layout.rimSplit2 != 0 && cur.motion_ws_layout.leanCount > 0;
        in.fused = fo.data != nullptr;
        in.leanFramesOk = lfg::lean_frames_ok(*prev, *curr, *mv);
        // (only while another lane has work queued or running -- a stream query each)
        for (size_t j = 0; j < ctx->lanes.size() && !in.othersBusy; ++j)
            if ((int)j != ctx->lane && ctx->lanes[j].stream && hipStreamQuery(ctx->lanes[j].stream) == hipErrorNotReady) in.othersBusy = true;
        in.slots = ctx->motion_slots;
        in.deviceCus = ctx->device_cus;
        in.commCus = ctx->comm_cus;
        const lfg::MotionCall call = lfg::motion_call_policy(v, in, ctx->knobs);
        cur.motion_ws_layout.lastLean = call.lean ? 1 : 0;
        ctx->motion_last_tier = fo.data ? 0 : call.tier;
        e = lfg::launch_motion_prefiltered_8_16(cur.stream, *prev, *curr, *mv, cur.motion_ws.data, cur.motion_ws_layout, cur.motion_units,
                                                rank2scan, order32, order32 + lfg::kMotionTableWords,
                                                ctx->motion_tables + 6 * lfg::kMotionTableWords, ctx->motion_hints, ctx->lanes.size() >= 2, fo,
                                                call.lean, call.deliverWord ? v.pinned : nullptr, call.groupsCap, call.expectNoFallback, ctx->knobs,
                                                ctx->semantics == 0, call.tier);
        if (e == hipSuccess && call.awaitVerdict) {
            e = hipEventRecord(v.event, cur.stream); v.pending = true;
            v.launchedOn = call.launchedOn;
        }
    }
    else if (tiled) e = lfg::launch_motion_tiled_8_16(ctx->cur().stream, *prev, *curr, *mv, nullptr, rank2scan, nullptr, nullptr, fo);
    else e = lfg::launch_motion_generic(ctx->cur().stream, *prev, *curr, *mv, block_size, R, ctx->semantics != 0);
    if (e != hipSuccess) return fail_hip(ctx, e, "motion kernel launch");
    if (fusedDone) *fusedDone = fo.data != nullptr;
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_last_variant(const lfg_context *ctx) { return ctx ? ctx->motion_last_tier : -1; }

LFG_EXPORT int lfg_motion(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *mv,
                          int block_size, float search_radius) {
    return motion_run(ctx, prev, curr, mv, block_size, search_radius, nullptr, nullptr);
}

LFG_EXPORT int lfg_set_semantics(lfg_context *ctx, int semantics) {
    if (!ctx || (semantics != LFG_SEMANTICS_REFERENCE && semantics != LFG_SEMANTICS_INTENDED))
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_semantics: unknown semantics");
    ctx->semantics = semantics;
    return LFG_OK;
}

LFG_EXPORT int lfg_set_motion_mode(lfg_context *ctx, int mode) {
    if (!ctx || (mode != LFG_MOTION_PREFILTERED && mode != LFG_MOTION_EXACT_ONLY))
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_motion_mode: unknown mode");
    ctx->motion_mode = mode;
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_pyramid(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *mv,
                                  int levels, int coarse_radius, int refine_radius) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(mv, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_pyramid: prev/curr must be RGBA8 and mv MV_S8X2, all non-empty");
    if (!same_size(prev, curr) || !same_size(curr, mv))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_pyramid: prev, curr and mv differ in size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u || mv->pitch % 2u || (uintptr_t)mv->data % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_pyramid: RGBA8 frames must be 4-byte aligned and mv 2-byte aligned");
    if (levels < 1 || levels > lfg::kPyramidMaxLevels || coarse_radius < 1 || coarse_radius > 32 || refine_radius < 1 || refine_radius > 4)
        return fail(ctx, LFG_ERR_UNSUPPORTED, "lfg_motion_pyramid: need 1 <= levels <= 4, 1 <= coarse_radius <= 32, 1 <= refine_radius <= 4");
    if (coarse_radius * (1 << levels) + refine_radius * ((1 << levels) - 1) > 127)
        return fail(ctx, LFG_ERR_UNSUPPORTED, "lfg_motion_pyramid: coarse_radius * 2^levels + refine_radius * (2^levels - 1) exceeds 127");
    lfg_lane_state &cur = ctx->cur();
    lfg::PyramidLayout layout;
    const size_t bytes = lfg::pyramid_workspace_bytes(curr->width, curr->height, levels, &layout);
    int rc = lane_buffer_grow(ctx, cur.pyramid_ws, bytes, "hipMalloc((void **)&cur.pyramid_ws, bytes)");
    if (rc != LFG_OK) return rc;
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e = lfg::launch_motion_pyramid(cur.stream, *prev, *curr, *mv, levels, coarse_radius, refine_radius, cur.pyramid_ws.data, layout);
    if (e != hipSuccess) return fail_hip(ctx, e, "pyramid motion kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_motion_estimator(lfg_context *ctx, int estimator) {
    if (!ctx || (estimator != LFG_ESTIMATOR_FULL_SEARCH && estimator != LFG_ESTIMATOR_PYRAMID))
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_motion_estimator: unknown estimator");
    ctx->estimator = estimator;
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_workspace_size(lfg_context *ctx, uint32_t width, uint32_t height, uint64_t *out_bytes) {
    if (!ctx) return LFG_ERR_INVALID;
    if (!out_bytes || width == 0 || height == 0 || width > 32768u || height > 32768u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_workspace_size: null output or a frame size outside 1..32768");
    if (ctx->motion_slots == 0) ctx->motion_slots = lfg::prefilter_slots();
    *out_bytes = (uint64_t)lfg::motion_workspace_bytes(width, height, ctx->motion_slots, motion_rim_split(ctx), motion_rim_split_lean(ctx), nullptr);
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_plan(const lfg_context *ctx, int *out_rim_split, int *out_workgroups) {
    if (!ctx) return LFG_ERR_INVALID;
    if (out_rim_split) *out_rim_split = motion_rim_split(ctx);
    if (out_workgroups) *out_workgroups = lfg::persistent_grid_most(ctx->motion_slots, ctx->device_cus, ctx->comm_cus);
    return LFG_OK;
}

// Reporting only: how many 16-row segments the prefilter of the last lfg_motion left to the resolve kernel, of how many the
// frame has (64 x 64 tiles x 4).  A segment is listed once; tests hold the list to that.
LFG_EXPORT int lfg_motion_open_segments(lfg_context *ctx, uint32_t *out_open, uint32_t *out_segments) {
    if (!ctx) return LFG_ERR_INVALID;
    lfg_lane_state &cur = ctx->cur();
    if (!out_open || !out_segments) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_open_segments: NULL argument");
    if (!cur.motion_ws.data || cur.motion_ws_w == 0) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_open_segments: the prefiltered path has not run");
    LFG_HIP(ctx, hipStreamSynchronize(cur.stream));
    const uint32_t tx = (cur.motion_ws_w + 55u) / 56u, ty = (cur.motion_ws_h + 63u) / 64u;      // (prefilter tiles: 56 x 64 pixels)
    uint32_t open = 0;
    LFG_HIP(ctx, hipMemcpy(&open, cur.motion_ws.data + cur.motion_ws_layout.ctrl + lfg::kCtrlOpenCount * sizeof(uint32_t), sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_open = open;
    *out_segments = tx * ty * 4u;
    return LFG_OK;
}

// Reporting only: how many entries of the run-time queue the whole tiles of the last lfg_motion asked for -- one per four parts of a
// segment handed over -- and how many the queue is laid out for (a call whose segments go in four parts uses half of them).  More
// asked for than there is room: the rest was searched in place.  Zero at frame sizes whose every tile is shared between units
// (prefilter_plan: fewer tiles than half the slots): only a unit that holds a whole tile hands a segment over.
LFG_EXPORT int lfg_motion_hand_over_stats(lfg_context *ctx, uint32_t *out_entries_asked, uint32_t *out_entries_room) {
    if (!ctx) return LFG_ERR_INVALID;
    lfg_lane_state &cur = ctx->cur();
    if (!out_entries_asked || !out_entries_room) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_hand_over_stats: NULL argument");
    if (!cur.motion_ws.data || cur.motion_ws_w == 0) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_hand_over_stats: the prefiltered path has not run");
    LFG_HIP(ctx, hipStreamSynchronize(cur.stream));
    uint32_t asked = 0;
    LFG_HIP(ctx, hipMemcpy(&asked, cur.motion_ws.data + cur.motion_ws_layout.queueCount, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_entries_asked = asked;
    *out_entries_room = (uint32_t)cur.motion_ws_layout.queueCap;
    return LFG_OK;
}

// Reporting only: did the selected lane's last lfg_motion go through the lean kernel (csrc/motion_lean.hip), how many whole
// interior tiles are listed for it at this frame size, and in how many of them it left a segment to the persistent kernel.
LFG_EXPORT int lfg_motion_lean_stats(lfg_context *ctx, int *out_used, uint32_t *out_tiles, uint32_t *out_tiles_left) {
    if (!ctx) return LFG_ERR_INVALID;
    lfg_lane_state &cur = ctx->cur();
    if (!out_used || !out_tiles || !out_tiles_left) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_lean_stats: NULL argument");
    if (!cur.motion_ws.data || cur.motion_ws_w == 0) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_lean_stats: the prefiltered path has not run");
    LFG_HIP(ctx, hipStreamSynchronize(cur.stream));
    uint32_t left = 0;
    LFG_HIP(ctx, hipMemcpy(&left, cur.motion_ws.data + cur.motion_ws_layout.ctrl + lfg::kCtrlHardCount * sizeof(uint32_t), sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_used = cur.motion_ws_layout.lastLean;
    *out_tiles = (uint32_t)cur.motion_ws_layout.leanCount;
    *out_tiles_left = cur.motion_ws_layout.lastLean ? left : 0u;
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_strip_stats(lfg_context *ctx, uint32_t *out_rows, uint32_t *out_columns) {
    if (!ctx) return LFG_ERR_INVALID;
    lfg_lane_state &cur = ctx->cur();
    if (!out_rows || !out_columns) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_strip_stats: NULL argument");
    if (!cur.motion_ws.data || cur.motion_ws_w == 0) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_strip_stats: the prefiltered path has not run");
    LFG_HIP(ctx, hipStreamSynchronize(cur.stream));
    std::vector<uint32_t> t((size_t)cur.motion_ws_h + cur.motion_ws_w);
    LFG_HIP(ctx, hipMemcpy(t.data(), cur.motion_ws.data + cur.motion_ws_layout.colBand, t.size() * 4, hipMemcpyDeviceToHost));
    uint32_t rows = 0, cols = 0;
    for (uint32_t y = 0; y < cur.motion_ws_h; ++y) rows += t[y] != 0u;
    for (uint32_t x = 0; x < cur.motion_ws_w; ++x) cols += t[cur.motion_ws_h + x] != 0u;
    *out_rows = rows; *out_columns = cols;
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_prediction_stats(const lfg_context *ctx, uint64_t *out_verdicts, uint64_t *out_lean_wrong,
                                           uint64_t *out_grid_wrong, uint64_t *out_second_pass_wrong) {
    if (!ctx) return LFG_ERR_INVALID;
    if (out_verdicts) *out_verdicts = ctx->pred_verdicts;
    if (out_lean_wrong) *out_lean_wrong = ctx->pred_lean_wrong;
    if (out_grid_wrong) *out_grid_wrong = ctx->pred_grid_wrong;
    if (out_second_pass_wrong) *out_second_pass_wrong = ctx->pred_second_wrong;
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_last_stats(lfg_context *ctx, uint32_t *out_tiles, uint32_t *out_fallback_tiles,
                                     double *out_mean_recorded) {
    if (!ctx) return LFG_ERR_INVALID;
    lfg_lane_state &cur = ctx->cur();
    if (!cur.motion_ws.data || cur.motion_ws_w == 0) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_last_stats: the prefiltered path has not run");
    LFG_HIP(ctx, hipStreamSynchronize(cur.stream));
    const uint32_t tx = (cur.motion_ws_w + 63u) / 64u, ty = (cur.motion_ws_h + 63u) / 64u;
    std::vector<uint32_t> flags((size_t)tx * ty);
    LFG_HIP(ctx, hipMemcpy(flags.data(), cur.motion_ws.data + cur.motion_ws_layout.tileFlags, flags.size() * 4, hipMemcpyDeviceToHost));
    uint32_t fb = 0;
    for (uint32_t f : flags) fb += f != 0u;
    if (ctx->knobs.debug) {
        uint32_t handed[2] = {0, 0};
        LFG_HIP(ctx, hipMemcpy(handed, cur.motion_ws.data + cur.motion_ws_layout.queueCount, 8, hipMemcpyDeviceToHost));
        fprintf(stderr, "lfg: motion prefilter: %u requests to hand a segment over (room for %d), %u tiles flagged for the exact kernel\n",
                handed[0], cur.motion_ws_layout.queueCap, handed[1]);
        uint32_t lean[2] = {0, 0};
        LFG_HIP(ctx, hipMemcpy(lean, cur.motion_ws.data + cur.motion_ws_layout.ctrl + lfg::kCtrlLeanSettled * sizeof(uint32_t), 8, hipMemcpyDeviceToHost));
        uint32_t flags[3] = {0, 0, 0};
        LFG_HIP(ctx, hipMemcpy(flags, cur.motion_ws.data + cur.motion_ws_layout.orderFlags, 12, hipMemcpyDeviceToHost));
        fprintf(stderr, "lfg: lean kernel: %d tiles listed, %u segments settled, %u left to the generic kernel (counted in -DLFG_LEAN_STATS builds); order flags: hand-over %u, hints %u, lean %u (sample blocks with a close match %u, with an exact one %u)\n",
                cur.motion_ws_layout.leanCount, lean[0], lean[1], flags[0], flags[1], lfg::verdict_lean(flags[2]) ? 1u : 0u, lfg::verdict_close(flags[2]), lfg::verdict_exact(flags[2]));
    }
    if (ctx->knobs.debugDyn) {       // the deepest private lists of the handed-over segments: block (4 x queue slot + wave), pixel, records
        uint32_t handed[2] = {0, 0};
        LFG_HIP(ctx, hipMemcpy(handed, cur.motion_ws.data + cur.motion_ws_layout.queueCount, 8, hipMemcpyDeviceToHost));
        const size_t blocks = (size_t)std::min<uint32_t>(handed[0], (uint32_t)cur.motion_ws_layout.queueCap) * 4u, per = 16u * 56u;
        std::vector<uint32_t> dc(blocks * per);
        if (!dc.empty()) LFG_HIP(ctx, hipMemcpy(dc.data(), cur.motion_ws.data + cur.motion_ws_layout.dynCount, dc.size() * 4, hipMemcpyDeviceToHost));
        size_t hist[40] = {0};
        int dumped = 0;
        const uint32_t deep = (uint32_t)ctx->knobs.debugDynDeep;
        for (size_t i = 0; i < dc.size(); ++i) {
            ++hist[std::min<uint32_t>(dc[i], 39u)];
            if (dc[i] > deep) {
                fprintf(stderr, "lfg: dyn list block %zu (part %zu of its segment) pixel %zu (row %zu, column %zu): %u records\n", i / per, (i / per) % 8u, i % per, (i % per) / 56u, (i % per) % 56u, dc[i]);
                if (dumped++ < 6) {      // the records themselves: lower bound of the cost and the candidate's rank, in the order they were recorded
                    const size_t blk = i / per, row = (i % per) / 56u, col = (i % per) % 56u;
                    const int K = cur.motion_ws_layout.listDyn;
                    for (int k = 0; k < std::min<int>((int)dc[i], K); ++k) {
                        uint32_t rec = 0; float thr = 0.f;
                        (void)hipMemcpy(&rec, cur.motion_ws.data + cur.motion_ws_layout.dynList + (((blk * 16u + row) * (size_t)K + (size_t)k) * 56u + col) * 4u, 4, hipMemcpyDeviceToHost);
                        (void)hipMemcpy(&thr, cur.motion_ws.data + cur.motion_ws_layout.dynUmin + ((blk * 16u + row) * 56u + col) * 4u, 4, hipMemcpyDeviceToHost);
                        const uint32_t bits = (rec >> 11) << 10; float c; memcpy(&c, &bits, 4);
                        fprintf(stderr, "      record %2d: cost >= %.3f rank %4u (dx %+d, dy %+d)%s\n", k, c, rec & 0x7FFu, (int)((rec & 0x7FFu) % 33u) - 16, (int)((rec & 0x7FFu) / 33u) - 16, k == 0 ? "" : "");
                        if (k + 1 == std::min<int>((int)dc[i], K)) fprintf(stderr, "      final threshold %.3f\n", thr);
                    }
                }
            }
        }
        {   // which segments under the flagged tiles were handed over
            const uint32_t ptx = (cur.motion_ws_w + 55u) / 56u, pty = (cur.motion_ws_h + 63u) / 64u;
            std::vector<uint32_t> sm((size_t)ptx * pty * 4u);
            LFG_HIP(ctx, hipMemcpy(sm.data(), cur.motion_ws.data + cur.motion_ws_layout.segMap, sm.size() * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < flags.size(); ++i) if (flags[i]) {
                const uint32_t fx = (uint32_t)(i % tx), fy = (uint32_t)(i / tx);
                for (uint32_t px = fx * 64u / 56u; px <= std::min(ptx - 1u, (fx * 64u + 63u) / 56u); ++px)
                    for (uint32_t sg = 0; sg < 4u; ++sg)
                        fprintf(stderr, "lfg: flagged tile (%u,%u) flag %#x: prefilter tile (%u,%u) segment %u segMap %#x\n", fx, fy, flags[i], px, fy, sg, sm[((size_t)fy * ptx + px) * 4u + sg]);
            }
        }
        for (size_t b = 0; b < blocks; ++b) {      // blocks nobody wrote counts into: their workgroup gave up (or the segment settled)
            bool any = false;
            for (size_t i = 0; i < per && !any; ++i) any = dc[b * per + i] != 0u;
            if (!any) fprintf(stderr, "lfg: dyn block %zu (part %zu) holds no counts\n", b, b % 8u);
        }
        {
            double sum[8] = {0}; size_t n8[8] = {0};
            for (size_t i = 0; i < dc.size(); ++i) { sum[(i / per) % 8u] += dc[i]; ++n8[(i / per) % 8u]; }
            fprintf(stderr, "lfg: mean records per pixel by part:");
            for (int k = 0; k < 8; ++k) fprintf(stderr, " %.2f", n8[k] ? sum[k] / n8[k] : 0.0);
            fprintf(stderr, "\n");
        }
        fprintf(stderr, "lfg: dyn list depths over %zu pixel-parts:", dc.size());
        for (int k = 0; k < 40; ++k) if (hist[k]) fprintf(stderr, " %d:%zu", k, hist[k]);
        fprintf(stderr, "\n");
    }
    if (ctx->knobs.debug)
        for (size_t i = 0; i < flags.size(); ++i)
            if (flags[i]) fprintf(stderr, "lfg: motion fallback tile (%zu, %zu)\n", i % tx, i / tx);
    if (out_tiles) *out_tiles = tx * ty;
    if (out_fallback_tiles) *out_fallback_tiles = fb;
    if (out_mean_recorded) {
        const size_t px = (size_t)cur.motion_ws_w * cur.motion_ws_h;
        std::vector<uint32_t> cnt(px);
        LFG_HIP(ctx, hipMemcpy(cnt.data(), cur.motion_ws.data + cur.motion_ws_layout.count, px * 4, hipMemcpyDeviceToHost));
        // (tiles whose candidates were shared between several workgroups keep their counts elsewhere: left out)
        const lfg::PrefilterPlanHost plan = lfg::prefilter_plan(cur.motion_ws_w, cur.motion_ws_h, ctx->motion_slots,
                                                                cur.motion_ws_layout.lastLean ? cur.motion_ws_layout.rimSplit2 : cur.motion_ws_layout.rimSplit);
        // (a segment that settled all of its pixels in the prefilter wrote no counts: its pixels hold at most two records,
        //  counted as none here)
        std::vector<uint32_t> segDone((size_t)plan.tiles * 4u);
        LFG_HIP(ctx, hipMemcpy(segDone.data(), cur.motion_ws.data + cur.motion_ws_layout.segDone, segDone.size() * 4, hipMemcpyDeviceToHost));
        double sum = 0; size_t n = 0;
        for (uint32_t y = 0; y < cur.motion_ws_h; ++y)
            for (uint32_t x = 0; x < cur.motion_ws_w; ++x) {
                const size_t ptile = (size_t)(y / 64u) * (size_t)plan.tilesX + x / 56u;
                if (!flags[(size_t)(y / 64u) * tx + x / 64u] && plan.tileMap[ptile] == 0xFFFFFFFFu) {
                    sum += segDone[ptile * 4u + (y % 64u) / 16u] ? 0.0 : (double)cnt[(size_t)y * cur.motion_ws_w + x]; ++n;
                }
            }
        *out_mean_recorded = n ? sum / (double)n : 0.0;
    }
    return LFG_OK;
}

LFG_EXPORT int lfg_interpolate(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                               lfg_frame *out, float factor) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));          // the stream belongs to this device (multi-GPU hosts)
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) ||
        !frame_ok(mv, LFG_FORMAT_MV_S8X2) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate: bad frame (NULL, empty or wrong format)");
    if (!same_size(prev, curr) || !same_size(curr, mv) || !same_size(curr, out))
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate: frames differ in size");
    if ((prev->pitch | curr->pitch | out->pitch) % 4u || mv->pitch % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate: row pitch not a multiple of the pixel size");
    if (out->data == prev->data || out->data == curr->data)
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate: output aliases an input");
    lfg::InterpTables tb;
    int rc = interp_tables(ctx, (int)curr->width, (int)curr->height, &tb);
    if (rc != LFG_OK) return rc;
    StageTimer timer(ctx, LFG_STAGE_INTERPOLATE);
    hipError_t e = lfg::launch_interpolate(ctx->cur().stream, *prev, *curr, *mv, *out, factor, ctx->semantics != 0, tb);
    if (e != hipSuccess) return fail_hip(ctx, e, "interpolate kernel launch");
    return LFG_OK;
}

namespace {

// The full search as lfg_interpolate_frames[_multi] run it (frame_manager.cpp:332-333).
constexpr int kFramesBlockSize = 8;
constexpr float kFramesSearchRadius = 16.0f;

// The vectors the generated frames are made from, on the selected lane: the selected estimator's in mv_tmp, and with
// lfg_set_vector_refinement their refinement in mv_refined.  The estimator is enqueued before mv_refined is made: making
// a frame can wait for every lane.  With lfg_set_half_resolution_motion the estimator runs on both frames halved, into the
// lane's half-size temporaries, and lfg_motion_expand writes `estimated` from its vectors.
int frame_vectors_into(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame &estimated, lfg_frame &refined,
                       const lfg_frame **vectors) {
    int rc = lane_frame(ctx, estimated, curr->width, curr->height, LFG_FORMAT_MV_S8X2);
    if (rc != LFG_OK) return fail(ctx, rc, "Failed to create motion vectors frame");
    if (ctx->half_res_radius >= 0) {
        lfg_lane_state &cur = ctx->cur();
        const uint32_t hw = (curr->width + 1u) / 2u, hh = (curr->height + 1u) / 2u;
        rc = lane_frame(ctx, cur.half_prev, hw, hh, LFG_FORMAT_RGBA8_UNORM);
        if (rc == LFG_OK) rc = lane_frame(ctx, cur.half_curr, hw, hh, LFG_FORMAT_RGBA8_UNORM);
        if (rc == LFG_OK) rc = lane_frame(ctx, cur.mv_half, hw, hh, LFG_FORMAT_MV_S8X2);
        if (rc != LFG_OK) return fail(ctx, rc, "Failed to create the half-resolution motion frames");
        if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !same_size(prev, curr))
            return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames: prev and curr must be non-empty RGBA8 frames of one size");
        rc = lfg_frame_halve(ctx, prev, &cur.half_prev);
        if (rc == LFG_OK) rc = lfg_frame_halve(ctx, curr, &cur.half_curr);
        if (rc == LFG_OK)
            rc = ctx->estimator == LFG_ESTIMATOR_PYRAMID
                     ? lfg_motion_pyramid(ctx, &cur.half_prev, &cur.half_curr, &cur.mv_half, 1, 16, 2)
                     : lfg_motion(ctx, &cur.half_prev, &cur.half_curr, &cur.mv_half, kFramesBlockSize, kFramesSearchRadius);
        if (rc == LFG_OK) rc = lfg_motion_expand(ctx, prev, curr, &cur.mv_half, &estimated, ctx->half_res_radius);
    } else {
        rc = ctx->estimator == LFG_ESTIMATOR_PYRAMID ? lfg_motion_pyramid(ctx, prev, curr, &estimated, 2, 16, 2)
                                                     : lfg_motion(ctx, prev, curr, &estimated, kFramesBlockSize, kFramesSearchRadius);
    }
    if (rc != LFG_OK) return rc;
    *vectors = &estimated;
    if (ctx->refine_radius < 0) return LFG_OK;
    rc = lane_frame(ctx, refined, curr->width, curr->height, LFG_FORMAT_MV_S8X2);
    if (rc != LFG_OK) return fail(ctx, rc, "Failed to create refined motion vectors frame");
    *vectors = &refined;
    return lfg_motion_refine(ctx, prev, curr, &estimated, &refined, ctx->refine_radius);
}

int frame_vectors(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame **vectors) {
    lfg_lane_state &cur = ctx->cur();
    return frame_vectors_into(ctx, prev, curr, cur.mv_tmp, cur.mv_refined, vectors);
}

// lfg_set_bidirectional's conditions: where they hold, compensated_frames measures the pair the other way too and runs the
// bidirectional call in the compensated interpolator's place.
bool bidirectional_applies(const lfg_context *ctx) {
    return ctx->bidir_tolerance >= 0 && ctx->interpolator == LFG_INTERPOLATOR_COMPENSATED &&
           ctx->generation == LFG_GENERATION_INTERPOLATE && ctx->static_tolerance < 0;
}

int cut_fallback_check(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const void *device_stats,
                       int min_matched_permille, lfg_frame *const *outs, const float *factors, uint32_t count);
int compensated_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *vectors,
                       lfg_frame *const *outs, const float *factors, uint32_t count, bool multi);
int cut_fallback_enqueue(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const void *device_stats,
                         int min_matched_permille, lfg_frame *const *outs, const float *factors, uint32_t count);
bool frames_overlap(const lfg_frame *a, const lfg_frame *b);

// lfg_interpolate_frames[_multi] with lfg_set_cut_detection on: the vectors, their match statistics into the lane's record
// (and a copy of it on its way to the host, for lfg_last_pair_stats), the selected interpolator, then the fallback, which
// reads the record on the device.  Everything that can fail on an argument is checked before the first launch.
// With lfg_set_level_matching on as well, `prev` is the lane's levelled prev', `shown` the caller's prev -- what the checks
// look at and what a cut shows -- and `level_map` the lane's map, which takes every interpolated output to the levels of its
// time before the fallback runs; otherwise shown is prev and level_map NULL.
int levels_at_outputs(lfg_context *ctx, const void *level_map, lfg_frame *const *outs, const float *factors, uint32_t count);

int detecting_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *const *outs, const float *factors,
                     uint32_t count, bool multi, const lfg_frame *shown, const void *level_map) {
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    lfg::CutDetectState &cut = ctx->cur().cut;
    if (!cut.device) LFG_HIP(ctx, hipMalloc((void **)&cut.device, sizeof(lfg_pair_stats)));
    if (!cut.pinned) LFG_HIP(ctx, hipHostMalloc((void **)&cut.pinned, sizeof(lfg_pair_stats), hipHostMallocDefault));
    if (!cut.event) LFG_HIP(ctx, hipEventCreateWithFlags(&cut.event, hipEventDisableTiming));
    const int permille = ctx->cut_permille;
    int rc = cut_fallback_check(ctx, shown, curr, cut.device, permille, outs, factors, count);
    if (rc != LFG_OK) return rc;
    const lfg_frame *vectors = nullptr;
    rc = frame_vectors(ctx, prev, curr, &vectors);
    if (rc != LFG_OK) return rc;
    rc = lfg_pair_match(ctx, prev, curr, vectors, ctx->match_sad, cut.device);
    if (rc != LFG_OK) return rc;
    LFG_HIP(ctx, hipMemcpyAsync(cut.pinned, cut.device, sizeof(lfg_pair_stats), hipMemcpyDeviceToHost, ctx->cur().stream));
    LFG_HIP(ctx, hipEventRecord(cut.event, ctx->cur().stream));
    cut.recorded = true;
    cut.permille = permille;
    if (ctx->interpolator == LFG_INTERPOLATOR_COMPENSATED)
        rc = compensated_frames(ctx, prev, curr, vectors, outs, factors, count, multi);
    else
        rc = multi ? lfg_interpolate_multi(ctx, prev, curr, vectors, outs, factors, count)
                   : lfg_interpolate(ctx, prev, curr, vectors, outs[0], factors[0]);
    if (rc != LFG_OK) return rc;
    if (ctx->generation == LFG_GENERATION_EXTRAPOLATE && ctx->interpolator == LFG_INTERPOLATOR_COMPENSATED) {
        float newest[LFG_MAX_FACTORS];                            // a cut repeats the newest frame: curr for every output
        for (uint32_t i = 0; i < count; ++i) newest[i] = 1.0f;
        return cut_fallback_enqueue(ctx, shown, curr, cut.device, permille, outs, newest, count);
    }
    if (level_map) {
        rc = levels_at_outputs(ctx, level_map, outs, factors, count);
        if (rc != LFG_OK) return rc;
    }
    return cut_fallback_enqueue(ctx, shown, curr, cut.device, permille, outs, factors, count);
}

// What lfg_interpolate_frames[_multi] run where neither cut detection nor the fused kernels apply: the vectors, then the
// selected interpolator.
int staged_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *const *outs, const float *factors,
                  uint32_t count, bool multi) {
    const lfg_frame *vectors = nullptr;
    int rc = frame_vectors(ctx, prev, curr, &vectors);
    if (rc != LFG_OK) return rc;
    if (ctx->interpolator == LFG_INTERPOLATOR_COMPENSATED) return compensated_frames(ctx, prev, curr, vectors, outs, factors, count, multi);
    return multi ? lfg_interpolate_multi(ctx, prev, curr, vectors, outs, factors, count)
                 : lfg_interpolate(ctx, prev, curr, vectors, outs[0], factors[0]);
}

// lfg_interpolate_frames[_multi] with lfg_set_level_matching on (include/linuxfg_hip.h has the six steps): everything that can
// fail on an argument is checked before the first launch -- lfg_cut_fallback's rules are the strictest any stage has for the
// frames, the compensated calls' the strictest for the factors -- then prev is levelled into the lane's prev', the call runs on
// prev' as it would have run on prev, and the interpolated outputs go to the levels of their own time.
int levelled_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *const *outs, const float *factors,
                    uint32_t count, bool multi) {
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    const char *name = multi ? "lfg_interpolate_frames_multi" : "lfg_interpolate_frames";
    const std::string n(name);
    if (!outs || !factors || count == 0 || count > LFG_MAX_FACTORS)
        return fail(ctx, LFG_ERR_INVALID, n + ": count must be in [1, LFG_MAX_FACTORS] and outs/factors non-NULL");
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !same_size(prev, curr))
        return fail(ctx, LFG_ERR_INVALID, n + ": prev and curr must be non-empty RGBA8 frames of one size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, n + ": RGBA8 frames must be 4-byte aligned");
    for (uint32_t i = 0; i < count; ++i) {
        const lfg_frame *o = outs[i];
        if (!frame_ok(o, LFG_FORMAT_RGBA8_UNORM) || !same_size(curr, o) || o->pitch % 4u || (uintptr_t)o->data % 4u)
            return fail(ctx, LFG_ERR_INVALID, n + ": bad output frame (NULL, empty, wrong format, size or alignment)");
        if (!std::isfinite(factors[i]) || factors[i] < 0.0f || factors[i] > 1.0f)
            return fail(ctx, LFG_ERR_INVALID, n + ": with level matching on every factor must be a finite number in [0, 1]");
        if (frames_overlap(o, prev) || frames_overlap(o, curr)) return fail(ctx, LFG_ERR_INVALID, n + ": an output overlaps an input");
        for (uint32_t j = 0; j < i; ++j)
            if (frames_overlap(outs[j], o)) return fail(ctx, LFG_ERR_INVALID, n + ": two outputs overlap each other");
    }
    lfg_lane_state &cur = ctx->cur();
    lfg::LevelMatchState &lv = cur.levels;
    constexpr size_t kRecord = sizeof(lfg_frame_histogram_stats), kHead = 3 * sizeof(uint64_t);
    if (!lv.device) LFG_HIP(ctx, hipMalloc((void **)&lv.device, 2 * kRecord + sizeof(lfg_levels_map)));
    if (!lv.pinned) LFG_HIP(ctx, hipHostMalloc((void **)&lv.pinned, kHead, hipHostMallocDefault));
    if (!lv.event) LFG_HIP(ctx, hipEventCreateWithFlags(&lv.event, hipEventDisableTiming));
    int rc = lane_frame(ctx, cur.levelled_prev, curr->width, curr->height, LFG_FORMAT_RGBA8_UNORM);
    if (rc != LFG_OK) return fail(ctx, rc, "Failed to create the levelled frame");
    void *const from = lv.device, *const to = lv.device + kRecord, *const map = lv.device + 2 * kRecord;
    rc = lfg_frame_histogram(ctx, prev, 0, from);
    if (rc == LFG_OK) rc = lfg_frame_histogram(ctx, curr, 0, to);
    if (rc == LFG_OK) rc = lfg_levels_match(ctx, from, to, ctx->level_shift16, map);
    if (rc == LFG_OK) rc = lfg_levels_apply(ctx, prev, &cur.levelled_prev, map, LFG_LEVELS_FORWARD, 0.0f);
    if (rc != LFG_OK) return rc;
    LFG_HIP(ctx, hipMemcpyAsync(lv.pinned, map, kHead, hipMemcpyDeviceToHost, cur.stream));
    LFG_HIP(ctx, hipEventRecord(lv.event, cur.stream));
    lv.recorded = true;
    const lfg_frame *levelled = &cur.levelled_prev;
    if (ctx->cut_permille >= 0) return detecting_frames(ctx, levelled, curr, outs, factors, count, multi, prev, map);
    rc = staged_frames(ctx, levelled, curr, outs, factors, count, multi);
    if (rc != LFG_OK) return rc;
    if (ctx->generation == LFG_GENERATION_EXTRAPOLATE && ctx->interpolator == LFG_INTERPOLATOR_COMPENSATED) return LFG_OK;
    return levels_at_outputs(ctx, map, outs, factors, count);
}

int levels_at_outputs(lfg_context *ctx, const void *level_map, lfg_frame *const *outs, const float *factors, uint32_t count) {
    for (uint32_t i = 0; i < count; ++i) {
        const int rc = lfg_levels_apply(ctx, outs[i], outs[i], level_map, LFG_LEVELS_AT, factors[i]);
        if (rc != LFG_OK) return rc;
    }
    return LFG_OK;
}

}  // namespace

LFG_EXPORT int lfg_interpolate_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                                      lfg_frame *out, float factor) {
    if (!ctx || !curr) return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames: NULL argument");
    if (pitch_too_large(prev) || pitch_too_large(curr) || pitch_too_large(out))     // before the lane's temporaries are made
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames: a pitch above 0x7fffffff");
    if (ctx->level_shift16 >= 0) {
        lfg_frame *const outs[1] = {out};
        return levelled_frames(ctx, prev, curr, outs, &factor, 1, false);
    }
    if (ctx->cut_permille >= 0) {
        lfg_frame *const outs[1] = {out};
        return detecting_frames(ctx, prev, curr, outs, &factor, 1, false, prev, nullptr);
    }
    // The fused motion kernels are the full search's and write the shader's interpolation: every other setting takes the stages.
    if (ctx->fuse_motion_interpolate && ctx->estimator == LFG_ESTIMATOR_FULL_SEARCH && ctx->refine_radius < 0 &&
        ctx->half_res_radius < 0 && ctx->interpolator == LFG_INTERPOLATOR_SHADER) {
        // The north-star order: the motion kernels write the generated frame from the vectors while they
        // hold them; the vector frame -- this call's temporary -- is not written at all.  `out` is checked as lfg_interpolate
        // checks it; whatever the fused path does not cover (see motion_run) goes on to lfg_interpolate.
        lfg_frame &mv = ctx->cur().mv_tmp;
        int rc = lane_frame(ctx, mv, curr->width, curr->height, LFG_FORMAT_MV_S8X2);
        if (rc != LFG_OK) return fail(ctx, rc, "Failed to create motion vectors frame");
        if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM) || !same_size(curr, out) || out->pitch % 4u)
            return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames: bad output frame (NULL, empty, wrong format, size or pitch)");
        if (out->data == prev->data || out->data == curr->data)
            return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames: the output aliases an input");
        lfg::FusedOut fo;
        fo.data = (uint8_t *)out->data; fo.pitch = (int)out->pitch; fo.t = factor; fo.intended = ctx->semantics != 0 ? 1 : 0; fo.storeMv = 0;
        bool done = false;
        rc = motion_run(ctx, prev, curr, &mv, kFramesBlockSize, kFramesSearchRadius, &fo, &done);
        if (rc != LFG_OK || done) return rc;
        return lfg_interpolate(ctx, prev, curr, &mv, out, factor);     // (the generic kernel ran: it wrote the vectors)
    }
    lfg_frame *const outs[1] = {out};
    return staged_frames(ctx, prev, curr, outs, &factor, 1, false);
}

LFG_EXPORT int lfg_interpolate_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                     lfg_frame *const *outs, const float *factors, uint32_t count) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!outs || !factors || count == 0 || count > LFG_MAX_FACTORS)
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: count must be in [1, LFG_MAX_FACTORS] and outs/factors non-NULL");
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(mv, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: bad frame (NULL, empty or wrong format)");
    if (!same_size(prev, curr) || !same_size(curr, mv))
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: frames differ in size");
    if ((prev->pitch | curr->pitch) % 4u || mv->pitch % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: row pitch not a multiple of the pixel size");
    for (uint32_t i = 0; i < count; ++i) {
        const lfg_frame *o = outs[i];
        if (!frame_ok(o, LFG_FORMAT_RGBA8_UNORM) || !same_size(curr, o) || o->pitch % 4u)
            return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: bad output frame (NULL, empty, wrong format, size or pitch)");
        if (o->data == prev->data || o->data == curr->data)
            return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: an output aliases an input");
        for (uint32_t j = 0; j < i; ++j)
            if (outs[j]->data == o->data) return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_multi: two outputs alias each other");
    }
    lfg::InterpTables tb;
    int rc = interp_tables(ctx, (int)curr->width, (int)curr->height, &tb);
    if (rc != LFG_OK) return rc;
    StageTimer timer(ctx, LFG_STAGE_INTERPOLATE);
    hipError_t e = lfg::launch_interpolate_multi(ctx->cur().stream, *prev, *curr, *mv, outs, factors, (int)count, ctx->semantics != 0, tb);
    if (e != hipSuccess) return fail_hip(ctx, e, "interpolate kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_interpolate_frames_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                                            lfg_frame *const *outs, const float *factors, uint32_t count) {
    if (!ctx || !curr) return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames_multi: NULL argument");
    bool too_large = pitch_too_large(prev) || pitch_too_large(curr);                // before the lane's temporaries are made
    for (uint32_t i = 0; outs && count <= LFG_MAX_FACTORS && i < count; ++i) too_large = too_large || pitch_too_large(outs[i]);
    if (too_large) return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_frames_multi: a pitch above 0x7fffffff");
    if (ctx->level_shift16 >= 0) return levelled_frames(ctx, prev, curr, outs, factors, count, true);
    if (ctx->cut_permille >= 0) return detecting_frames(ctx, prev, curr, outs, factors, count, true, prev, nullptr);
    return staged_frames(ctx, prev, curr, outs, factors, count, true);
}

// ---- motion-compensated interpolation (interpolate_mc.hip)

namespace {

// The bytes a frame's pixels span: from the first row's start to the last row's last pixel.
bool frames_overlap(const lfg_frame *a, const lfg_frame *b) {
    const uintptr_t a0 = (uintptr_t)a->data, b0 = (uintptr_t)b->data;
    const uintptr_t a1 = a0 + (size_t)a->pitch * (a->height - 1u) + (size_t)a->width * bytes_per_pixel(a->format);
    const uintptr_t b1 = b0 + (size_t)b->pitch * (b->height - 1u) + (size_t)b->width * bytes_per_pixel(b->format);
    return a0 < b1 && b0 < a1;
}

// The bytes a mask's pixels span against a frame's.
bool mask_overlaps(const lfg_mask *m, const lfg_frame *f) {
    const uintptr_t a0 = (uintptr_t)m->data, b0 = (uintptr_t)f->data;
    const uintptr_t a1 = a0 + (size_t)m->pitch * (m->height - 1u) + (size_t)m->width;
    const uintptr_t b1 = b0 + (size_t)f->pitch * (f->height - 1u) + (size_t)f->width * bytes_per_pixel(f->format);
    return a0 < b1 && b0 < a1;
}

bool mask_ok(const lfg_mask *m, const lfg_frame *like) {
    return m && m->data && m->width == like->width && m->height == like->height && m->pitch >= m->width;
}

// The four stages that project the vectors into the lane's key image: lfg_interpolate_compensated[_multi], with a mask
// lfg_interpolate_compensated_masked[_multi], lfg_extrapolate_compensated[_multi], whose factors are its `aheads`, and
// lfg_interpolate_compensated_bidirectional[_multi], whose mv is `fwd` and which alone takes `bwd` and `tolerance`.  And
// lfg_interpolate_compensated_subpel[_multi], whose mv is the quarter-pixel `mvq`: another format and alignment, a key image of
// its own with 64-bit words, and no fill plane.
enum class McKind { Plain, Masked, Extrapolate, Bidirectional, Subpel };

int compensated_run(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv, const lfg_mask *mask, McKind kind,
                    lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad, const char *name,
                    const lfg_frame *bwd = nullptr, int tolerance = 0, int sampling = LFG_SAMPLING_BILINEAR) {
    const bool masked = kind == McKind::Masked, bidir = kind == McKind::Bidirectional, subpel = kind == McKind::Subpel;
    const uint32_t mvFormat = subpel ? LFG_FORMAT_MV_S16X2_Q2 : LFG_FORMAT_MV_S8X2, mvAlign = subpel ? 4u : 2u;
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    const std::string n(name);
    if (!outs || !factors || count == 0 || count > LFG_MAX_FACTORS)
        return fail(ctx, LFG_ERR_INVALID, n + ": count must be in [1, LFG_MAX_FACTORS] and outs/factors non-NULL");
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(mv, mvFormat))
        return fail(ctx, LFG_ERR_INVALID, n + (subpel ? ": prev/curr must be RGBA8 and mvq MV_S16X2_Q2, all non-empty"
                                                      : ": prev/curr must be RGBA8 and mv MV_S8X2, all non-empty"));
    if (!same_size(prev, curr) || !same_size(curr, mv))
        return fail(ctx, LFG_ERR_INVALID, n + ": prev, curr and mv differ in size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u || mv->pitch % mvAlign || (uintptr_t)mv->data % mvAlign)
        return fail(ctx, LFG_ERR_INVALID, n + (subpel ? ": RGBA8 frames and mvq must be 4-byte aligned"
                                                      : ": RGBA8 frames must be 4-byte aligned and mv 2-byte aligned"));
    if (match_sad < 0 || match_sad > 1020) return fail(ctx, LFG_ERR_INVALID, n + ": match_sad must be in [0, 1020]");
    if (masked && !mask_ok(mask, curr))
        return fail(ctx, LFG_ERR_INVALID, n + ": mask must be non-NULL, of the frames' size, with pitch >= width");
    if (bidir && (!frame_ok(bwd, LFG_FORMAT_MV_S8X2) || !same_size(curr, bwd) || bwd->pitch % 2u || (uintptr_t)bwd->data % 2u))
        return fail(ctx, LFG_ERR_INVALID, n + ": bwd must be a non-empty, 2-byte aligned MV_S8X2 frame of the frames' size");
    if (bidir && (tolerance < 0 || tolerance > 64)) return fail(ctx, LFG_ERR_INVALID, n + ": tolerance must be in [0, 64]");
    for (uint32_t i = 0; i < count; ++i) {
        const lfg_frame *o = outs[i];
        if (!frame_ok(o, LFG_FORMAT_RGBA8_UNORM) || !same_size(curr, o) || o->pitch % 4u || (uintptr_t)o->data % 4u)
            return fail(ctx, LFG_ERR_INVALID, n + ": bad output frame (NULL, empty, wrong format, size or alignment)");
        if (!std::isfinite(factors[i]) || factors[i] < 0.0f || factors[i] > 1.0f)
            return fail(ctx, LFG_ERR_INVALID, n + ": every factor must be a finite number in [0, 1]");
        if (frames_overlap(o, prev) || frames_overlap(o, curr) || frames_overlap(o, mv) || (masked && mask_overlaps(mask, o)) ||
            (bidir && frames_overlap(o, bwd)))
            return fail(ctx, LFG_ERR_INVALID, n + ": an output aliases an input");
        for (uint32_t j = 0; j < i; ++j)
            if (frames_overlap(outs[j], o)) return fail(ctx, LFG_ERR_INVALID, n + ": two outputs alias each other");
    }
    lfg_lane_state &cur = ctx->cur();
    const size_t bytes = (size_t)curr->width * curr->height * 4u;
    int rc = subpel ? lane_buffer_grow(ctx, cur.mcq_keys, 2u * bytes, "hipMalloc((void **)&cur.mcq_keys, 2 * bytes)")
                    : lane_buffer_grow(ctx, cur.mc_keys, bytes, "hipMalloc((void **)&cur.mc_keys, bytes)");
    if (rc != LFG_OK) return rc;
    // lfg_set_hole_reach: the three interpolating kinds of whole-pixel vectors fill their holes from the lane's fill plane, made
    // per factor behind K
    // LFG_SAMPLING_BICUBIC (the plain and sub-pixel kinds alone): the walk, as no fill-plane variant of that sampling kernel is built
    const bool bicubic = sampling == LFG_SAMPLING_BICUBIC && (kind == McKind::Plain || subpel);
    const int reach = kind == McKind::Extrapolate || subpel || bicubic ? -1 : ctx->hole_reach;
    if (reach >= 1) {
        rc = lane_buffer_grow(ctx, cur.mc_fill, bytes, "hipMalloc((void **)&cur.mc_fill, bytes)");
        if (rc != LFG_OK) return rc;
    }
    uint32_t *const fill = reach >= 1 ? cur.mc_fill.as<uint32_t>() : nullptr, *const keys = cur.mc_keys.as<uint32_t>();
    unsigned long long *const keys64 = cur.mcq_keys.as<unsigned long long>();
    StageTimer timer(ctx, LFG_STAGE_INTERPOLATE);
    for (uint32_t i = 0; i < count; ++i) {                       // one key image (and one fill plane), reused in stream order
        hipError_t e = bicubic ? (subpel ? lfg::launch_interpolate_compensated_subpel_bicubic(cur.stream, *prev, *curr, *mv, *outs[i], factors[i], match_sad, keys64)
                                         : lfg::launch_interpolate_compensated_bicubic(cur.stream, *prev, *curr, *mv, *outs[i], factors[i], match_sad, keys))
                       : subpel ? lfg::launch_interpolate_compensated_subpel(cur.stream, *prev, *curr, *mv, *outs[i], factors[i], match_sad, keys64)
                       : masked ? lfg::launch_interpolate_compensated_masked(cur.stream, *prev, *curr, *mv, *mask, *outs[i], factors[i], match_sad, keys,
                                                                           fill, reach)
                       : kind == McKind::Extrapolate
                              ? lfg::launch_extrapolate_compensated(cur.stream, *prev, *curr, *mv, *outs[i], factors[i], match_sad, keys)
                       : bidir ? lfg::launch_interpolate_compensated_bidirectional(cur.stream, *prev, *curr, *mv, *bwd, *outs[i], factors[i],
                                                                                   match_sad, tolerance, keys, fill, reach)
                              : lfg::launch_interpolate_compensated(cur.stream, *prev, *curr, *mv, *outs[i], factors[i], match_sad, keys,
                                                                    fill, reach);
        if (e != hipSuccess) return fail_hip(ctx, e, kind == McKind::Extrapolate ? "compensated extrapolate kernel launch" : "compensated interpolate kernel launch");
    }
    return LFG_OK;
}

// Exactly where compensated_frames would run the plain kind with the walk: lfg_set_subpixel_vectors' conditions, and
// lfg_set_sampling's, which holds for the sub-pixel kind that then runs in its place too.
bool plain_walk_applies(const lfg_context *ctx) {
    return ctx->interpolator == LFG_INTERPOLATOR_COMPENSATED && ctx->generation == LFG_GENERATION_INTERPOLATE &&
           ctx->bidir_tolerance < 0 && ctx->static_tolerance < 0 && ctx->hole_reach < 0;
}
bool subpixel_applies(const lfg_context *ctx) { return ctx->subpel_radius >= 0 && plain_walk_applies(ctx); }
int sampling_effective(const lfg_context *ctx) { return plain_walk_applies(ctx) ? ctx->sampling : (int)LFG_SAMPLING_BILINEAR; }

// The compensated interpolation of lfg_interpolate_frames[_multi]: as it is, or with lfg_set_static_protection on the pair's
// static mask into the lane's temporary and the masked call in its place; under LFG_GENERATION_EXTRAPOLATE the extrapolation
// in the place of both.  Where lfg_set_bidirectional applies: the pair measured the other way as `vectors` were measured, into the
// lane's backward temporaries, and the bidirectional call in the compensated one's place.
int compensated_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *vectors,
                       lfg_frame *const *outs, const float *factors, uint32_t count, bool multi) {
    if (ctx->generation == LFG_GENERATION_EXTRAPOLATE)             // each factor is an `ahead`; static protection does not apply
        return compensated_run(ctx, prev, curr, vectors, nullptr, McKind::Extrapolate, outs, factors, count, ctx->match_sad,
                               multi ? "lfg_extrapolate_compensated_multi" : "lfg_extrapolate_compensated");
    if (bidirectional_applies(ctx)) {
        lfg_lane_state &cur = ctx->cur();
        const lfg_frame *backward = nullptr;
        const int rc = frame_vectors_into(ctx, curr, prev, cur.mv_bwd, cur.mv_bwd_refined, &backward);
        if (rc != LFG_OK) return rc;
        return compensated_run(ctx, prev, curr, vectors, nullptr, McKind::Bidirectional, outs, factors, count, ctx->match_sad,
                               multi ? "lfg_interpolate_compensated_bidirectional_multi" : "lfg_interpolate_compensated_bidirectional",
                               backward, ctx->bidir_tolerance);
    }
    if (subpixel_applies(ctx)) {                                   // the final integer field to quarter pixels, then the route that carries them
        lfg_lane_state &cur = ctx->cur();
        int rc = lane_frame(ctx, cur.mvq_tmp, curr->width, curr->height, LFG_FORMAT_MV_S16X2_Q2);
        if (rc != LFG_OK) return fail(ctx, rc, "Failed to create the quarter-pixel motion vectors frame");
        rc = lfg_motion_subpel(ctx, prev, curr, vectors, &cur.mvq_tmp, ctx->subpel_radius);
        if (rc != LFG_OK) return rc;
        return compensated_run(ctx, prev, curr, &cur.mvq_tmp, nullptr, McKind::Subpel, outs, factors, count, ctx->match_sad,
                               multi ? "lfg_interpolate_compensated_subpel_multi" : "lfg_interpolate_compensated_subpel", nullptr, 0,
                               sampling_effective(ctx));
    }
    if (ctx->static_tolerance < 0)                                 // (with a hole reach the effective sampling is bilinear)
        return compensated_run(ctx, prev, curr, vectors, nullptr, McKind::Plain, outs, factors, count, ctx->match_sad,
                               multi ? "lfg_interpolate_compensated_multi" : "lfg_interpolate_compensated", nullptr, 0,
                               sampling_effective(ctx));
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    lfg_lane_state &cur = ctx->cur();
    const size_t bytes = (size_t)curr->width * curr->height;
    int rc = lane_buffer_grow(ctx, cur.static_mask, bytes, "hipMalloc((void **)&cur.static_mask, bytes)");
    if (rc != LFG_OK) return rc;
    const lfg_mask mask{cur.static_mask.data, curr->width, curr->height, curr->width};
    rc = lfg_static_mask(ctx, prev, curr, ctx->static_tolerance, &mask);
    if (rc != LFG_OK) return rc;
    return compensated_run(ctx, prev, curr, vectors, &mask, McKind::Masked, outs, factors, count, ctx->match_sad,
                           multi ? "lfg_interpolate_compensated_masked_multi" : "lfg_interpolate_compensated_masked");
}

}  // namespace

LFG_EXPORT int lfg_interpolate_compensated(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                           lfg_frame *out, float factor, int match_sad) {
    lfg_frame *const outs[1] = {out};
    return compensated_run(ctx, prev, curr, mv, nullptr, McKind::Plain, outs, &factor, 1, match_sad, "lfg_interpolate_compensated");
}

LFG_EXPORT int lfg_interpolate_compensated_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                                 lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad) {
    return compensated_run(ctx, prev, curr, mv, nullptr, McKind::Plain, outs, factors, count, match_sad, "lfg_interpolate_compensated_multi");
}

// ---- the fill plane (hole_fill.hip)

LFG_EXPORT int lfg_hole_fill_plane(lfg_context *ctx, const lfg_frame *keys, int reach, int pass_static, lfg_frame *plane) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(keys, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(plane, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_hole_fill_plane: keys and plane must be non-empty RGBA8");
    if (!same_size(keys, plane)) return fail(ctx, LFG_ERR_INVALID, "lfg_hole_fill_plane: keys and plane differ in size");
    if ((keys->pitch | plane->pitch) % 4u || ((uintptr_t)keys->data | (uintptr_t)plane->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_hole_fill_plane: RGBA8 frames must be 4-byte aligned");
    if (frames_overlap(keys, plane)) return fail(ctx, LFG_ERR_INVALID, "lfg_hole_fill_plane: plane overlaps keys");
    if (reach < 1 || reach > LFG_HOLE_REACH_MAX)
        return fail(ctx, LFG_ERR_INVALID, "lfg_hole_fill_plane: reach must be in [1, LFG_HOLE_REACH_MAX]");
    if (pass_static != 0 && pass_static != 1) return fail(ctx, LFG_ERR_INVALID, "lfg_hole_fill_plane: pass_static must be 0 or 1");
    const hipError_t e = lfg::launch_hole_fill_plane(ctx->cur().stream, (const uint32_t *)keys->data, keys->pitch / 4u, (uint32_t *)plane->data,
                                                     plane->pitch / 4u, (int)keys->width, (int)keys->height, reach, pass_static != 0,
                                                     ctx->knobs.fillBand);
    if (e != hipSuccess) return fail_hip(ctx, e, "fill plane kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_hole_reach(lfg_context *ctx, int reach) {
    if (!ctx) return LFG_ERR_INVALID;
    if (reach != -1 && (reach < 1 || reach > LFG_HOLE_REACH_MAX))
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_hole_reach: reach must be -1 (off) or in [1, LFG_HOLE_REACH_MAX]");
    ctx->hole_reach = reach;
    return LFG_OK;
}

// ---- motion-compensated extrapolation (extrapolate_mc.hip)

LFG_EXPORT int lfg_extrapolate_compensated(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                           lfg_frame *out, float ahead, int match_sad) {
    lfg_frame *const outs[1] = {out};
    return compensated_run(ctx, prev, curr, mv, nullptr, McKind::Extrapolate, outs, &ahead, 1, match_sad, "lfg_extrapolate_compensated");
}

LFG_EXPORT int lfg_extrapolate_compensated_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                                 lfg_frame *const *outs, const float *aheads, uint32_t count, int match_sad) {
    return compensated_run(ctx, prev, curr, mv, nullptr, McKind::Extrapolate, outs, aheads, count, match_sad, "lfg_extrapolate_compensated_multi");
}

LFG_EXPORT int lfg_set_generation(lfg_context *ctx, int generation) {
    if (!ctx) return LFG_ERR_INVALID;
    if (generation != LFG_GENERATION_INTERPOLATE && generation != LFG_GENERATION_EXTRAPOLATE)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_generation: unknown generation");
    ctx->generation = generation;
    return LFG_OK;
}

// ---- bidirectional compensated interpolation (interpolate_bidir.hip)

LFG_EXPORT int lfg_interpolate_compensated_bidirectional(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                                                         const lfg_frame *fwd, const lfg_frame *bwd, lfg_frame *out, float factor,
                                                         int match_sad, int tolerance) {
    lfg_frame *const outs[1] = {out};
    return compensated_run(ctx, prev, curr, fwd, nullptr, McKind::Bidirectional, outs, &factor, 1, match_sad,
                           "lfg_interpolate_compensated_bidirectional", bwd, tolerance);
}

LFG_EXPORT int lfg_interpolate_compensated_bidirectional_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                                                               const lfg_frame *fwd, const lfg_frame *bwd, lfg_frame *const *outs,
                                                               const float *factors, uint32_t count, int match_sad, int tolerance) {
    return compensated_run(ctx, prev, curr, fwd, nullptr, McKind::Bidirectional, outs, factors, count, match_sad,
                           "lfg_interpolate_compensated_bidirectional_multi", bwd, tolerance);
}

LFG_EXPORT int lfg_motion_consistency(lfg_context *ctx, const lfg_frame *a, const lfg_frame *b, int tolerance, const lfg_mask *out) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(a, LFG_FORMAT_MV_S8X2) || !frame_ok(b, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_consistency: a and b must be non-empty MV_S8X2");
    if (!same_size(a, b)) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_consistency: a and b differ in size");
    if ((a->pitch | b->pitch) % 2u || ((uintptr_t)a->data | (uintptr_t)b->data) % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_consistency: MV_S8X2 frames must be 2-byte aligned");
    if (tolerance < 0 || tolerance > 64) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_consistency: tolerance must be in [0, 64]");
    if (!mask_ok(out, a))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_consistency: out must be non-NULL, of the fields' size, with pitch >= width");
    if (mask_overlaps(out, a) || mask_overlaps(out, b))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_consistency: out overlaps an input");
    hipError_t e = lfg::launch_motion_consistency(ctx->cur().stream, *a, *b, tolerance, *out);
    if (e != hipSuccess) return fail_hip(ctx, e, "motion consistency kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_bidirectional(lfg_context *ctx, int tolerance) {
    if (!ctx) return LFG_ERR_INVALID;
    if (tolerance < -1 || tolerance > 64)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_bidirectional: tolerance must be -1 (off) or in [0, 64]");
    ctx->bidir_tolerance = tolerance;
    return LFG_OK;
}

// ---- static-overlay protection (static_mask.hip, interpolate_mc.hip)

LFG_EXPORT int lfg_static_mask(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, int tolerance, const lfg_mask *out) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_static_mask: prev and curr must be non-empty RGBA8");
    if (!same_size(prev, curr)) return fail(ctx, LFG_ERR_INVALID, "lfg_static_mask: prev and curr differ in size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_static_mask: RGBA8 frames must be 4-byte aligned");
    if (tolerance < 0 || tolerance > 1020) return fail(ctx, LFG_ERR_INVALID, "lfg_static_mask: tolerance must be in [0, 1020]");
    if (!mask_ok(out, curr))
        return fail(ctx, LFG_ERR_INVALID, "lfg_static_mask: out must be non-NULL, of the frames' size, with pitch >= width");
    if (mask_overlaps(out, prev) || mask_overlaps(out, curr))
        return fail(ctx, LFG_ERR_INVALID, "lfg_static_mask: out overlaps an input");
    hipError_t e = lfg::launch_static_mask(ctx->cur().stream, *prev, *curr, tolerance, *out);
    if (e != hipSuccess) return fail_hip(ctx, e, "static mask kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_interpolate_compensated_masked(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                                  const lfg_mask *mask, lfg_frame *out, float factor, int match_sad) {
    lfg_frame *const outs[1] = {out};
    return compensated_run(ctx, prev, curr, mv, mask, McKind::Masked, outs, &factor, 1, match_sad, "lfg_interpolate_compensated_masked");
}

LFG_EXPORT int lfg_interpolate_compensated_masked_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                                        const lfg_mask *mask, lfg_frame *const *outs, const float *factors, uint32_t count,
                                                        int match_sad) {
    return compensated_run(ctx, prev, curr, mv, mask, McKind::Masked, outs, factors, count, match_sad, "lfg_interpolate_compensated_masked_multi");
}

LFG_EXPORT int lfg_set_static_protection(lfg_context *ctx, int tolerance) {
    if (!ctx) return LFG_ERR_INVALID;
    if (tolerance < -1 || tolerance > 1020)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_static_protection: tolerance must be -1 (off) or in [0, 1020]");
    ctx->static_tolerance = tolerance;
    return LFG_OK;
}

LFG_EXPORT int lfg_set_interpolator(lfg_context *ctx, int interpolator, int match_sad) {
    if (!ctx) return LFG_ERR_INVALID;
    if (interpolator != LFG_INTERPOLATOR_SHADER && interpolator != LFG_INTERPOLATOR_COMPENSATED)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_interpolator: unknown interpolator");
    if (match_sad < 0 || match_sad > 1020) return fail(ctx, LFG_ERR_INVALID, "lfg_set_interpolator: match_sad must be in [0, 1020]");
    ctx->interpolator = interpolator;
    ctx->match_sad = match_sad;
    return LFG_OK;
}

// ---- per-pixel vector refinement (motion_refine.hip)

LFG_EXPORT int lfg_motion_refine(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv_in,
                                 lfg_frame *mv_out, int radius) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) ||
        !frame_ok(mv_in, LFG_FORMAT_MV_S8X2) || !frame_ok(mv_out, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_refine: prev/curr must be RGBA8 and mv_in/mv_out MV_S8X2, all non-empty");
    if (!same_size(prev, curr) || !same_size(curr, mv_in) || !same_size(curr, mv_out))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_refine: prev, curr, mv_in and mv_out differ in size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u ||
        (mv_in->pitch | mv_out->pitch) % 2u || ((uintptr_t)mv_in->data | (uintptr_t)mv_out->data) % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_refine: RGBA8 frames must be 4-byte aligned and mv 2-byte aligned");
    if (frames_overlap(mv_out, prev) || frames_overlap(mv_out, curr) || frames_overlap(mv_out, mv_in))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_refine: mv_out overlaps an input (it cannot run in place)");
    if (radius < 0 || radius > 2) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_refine: radius must be in [0, 2]");
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e = lfg::launch_motion_refine(ctx->cur().stream, *prev, *curr, *mv_in, *mv_out, radius);
    if (e != hipSuccess) return fail_hip(ctx, e, "motion refine kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_vector_refinement(lfg_context *ctx, int radius) {
    if (!ctx) return LFG_ERR_INVALID;
    if (radius < -1 || radius > 2) return fail(ctx, LFG_ERR_INVALID, "lfg_set_vector_refinement: radius must be -1 (off) or in [0, 2]");
    ctx->refine_radius = radius;
    return LFG_OK;
}

// ---- half-resolution motion (motion_expand.hip)

LFG_EXPORT int lfg_frame_halve(lfg_context *ctx, const lfg_frame *in, lfg_frame *out) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(in, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_halve: in and out must be non-empty RGBA8");
    if (out->width != (in->width + 1u) / 2u || out->height != (in->height + 1u) / 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_halve: out must be ceil(W / 2) x ceil(H / 2)");
    if ((in->pitch | out->pitch) % 4u || ((uintptr_t)in->data | (uintptr_t)out->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_halve: RGBA8 frames must be 4-byte aligned");
    if (frames_overlap(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_halve: out overlaps in");
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e = lfg::launch_frame_halve(ctx->cur().stream, *in, *out);
    if (e != hipSuccess) return fail_hip(ctx, e, "frame halve kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_motion_expand(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv_low,
                                 lfg_frame *mv_out, int radius) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) ||
        !frame_ok(mv_low, LFG_FORMAT_MV_S8X2) || !frame_ok(mv_out, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_expand: prev/curr must be RGBA8 and mv_low/mv_out MV_S8X2, all non-empty");
    if (!same_size(prev, curr) || !same_size(curr, mv_out))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_expand: prev, curr and mv_out differ in size");
    if (mv_low->width != (curr->width + 1u) / 2u || mv_low->height != (curr->height + 1u) / 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_expand: mv_low must be ceil(W / 2) x ceil(H / 2)");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u ||
        (mv_low->pitch | mv_out->pitch) % 2u || ((uintptr_t)mv_low->data | (uintptr_t)mv_out->data) % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_expand: RGBA8 frames must be 4-byte aligned and mv 2-byte aligned");
    if (frames_overlap(mv_out, prev) || frames_overlap(mv_out, curr) || frames_overlap(mv_out, mv_low))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_expand: mv_out overlaps an input");
    if (radius < 0 || radius > 2) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_expand: radius must be in [0, 2]");
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e = lfg::launch_motion_expand(ctx->cur().stream, *prev, *curr, *mv_low, *mv_out, radius);
    if (e != hipSuccess) return fail_hip(ctx, e, "motion expand kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_half_resolution_motion(lfg_context *ctx, int radius) {
    if (!ctx) return LFG_ERR_INVALID;
    if (radius < -1 || radius > 2)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_half_resolution_motion: radius must be -1 (off) or in [0, 2]");
    ctx->half_res_radius = radius;
    return LFG_OK;
}

// ---- quarter-pixel vectors (motion_subpel.hip, interpolate_subpel.hip)

LFG_EXPORT int lfg_motion_subpel(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv_in,
                                 lfg_frame *mvq_out, int radius) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) ||
        !frame_ok(mv_in, LFG_FORMAT_MV_S8X2) || !frame_ok(mvq_out, LFG_FORMAT_MV_S16X2_Q2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_subpel: prev/curr must be RGBA8, mv_in MV_S8X2 and mvq_out MV_S16X2_Q2, all non-empty");
    if (!same_size(prev, curr) || !same_size(curr, mv_in) || !same_size(curr, mvq_out))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_subpel: prev, curr, mv_in and mvq_out differ in size");
    if ((prev->pitch | curr->pitch | mvq_out->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data | (uintptr_t)mvq_out->data) % 4u ||
        mv_in->pitch % 2u || (uintptr_t)mv_in->data % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_subpel: RGBA8 frames and mvq_out must be 4-byte aligned and mv_in 2-byte aligned");
    if (frames_overlap(mvq_out, prev) || frames_overlap(mvq_out, curr) || frames_overlap(mvq_out, mv_in))
        return fail(ctx, LFG_ERR_INVALID, "lfg_motion_subpel: mvq_out overlaps an input");
    if (radius < 0 || radius > 2) return fail(ctx, LFG_ERR_INVALID, "lfg_motion_subpel: radius must be in [0, 2]");
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e = lfg::launch_motion_subpel(ctx->cur().stream, *prev, *curr, *mv_in, *mvq_out, radius);
    if (e != hipSuccess) return fail_hip(ctx, e, "motion subpel kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_interpolate_compensated_subpel(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mvq,
                                                  lfg_frame *out, float factor, int match_sad) {
    lfg_frame *const outs[1] = {out};
    return compensated_run(ctx, prev, curr, mvq, nullptr, McKind::Subpel, outs, &factor, 1, match_sad, "lfg_interpolate_compensated_subpel");
}

LFG_EXPORT int lfg_interpolate_compensated_subpel_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mvq,
                                                        lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad) {
    return compensated_run(ctx, prev, curr, mvq, nullptr, McKind::Subpel, outs, factors, count, match_sad, "lfg_interpolate_compensated_subpel_multi");
}

LFG_EXPORT int lfg_set_subpixel_vectors(lfg_context *ctx, int radius) {
    if (!ctx) return LFG_ERR_INVALID;
    if (radius < -1 || radius > 2) return fail(ctx, LFG_ERR_INVALID, "lfg_set_subpixel_vectors: radius must be -1 (off) or in [0, 2]");
    ctx->subpel_radius = radius;
    return LFG_OK;
}

// ---- the bicubic fetch (interpolate_bicubic.hip, lfg_bicubic.hpp)

LFG_EXPORT int lfg_sampling_weights(int16_t weights[256]) {
    if (!weights) return LFG_ERR_INVALID;
    for (int phi = 0; phi < lfg::kBicubicPhases; ++phi) {
        const lfg::BicubicRow row = lfg::bicubic_row(phi);
        for (int k = 0; k < 4; ++k) weights[4 * phi + k] = (int16_t)row.w[k];
    }
    return LFG_OK;
}

namespace {

// mv's format picks the route; everything else is that kind's, through compensated_run.
int compensated_sampled(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv, lfg_frame *const *outs,
                        const float *factors, uint32_t count, int match_sad, int sampling, const char *name) {
    if (!ctx) return LFG_ERR_INVALID;
    if (sampling != LFG_SAMPLING_BILINEAR && sampling != LFG_SAMPLING_BICUBIC)
        return fail(ctx, LFG_ERR_INVALID, std::string(name) + ": sampling must be LFG_SAMPLING_BILINEAR or LFG_SAMPLING_BICUBIC");
    const McKind kind = mv && mv->format == LFG_FORMAT_MV_S16X2_Q2 ? McKind::Subpel : McKind::Plain;
    return compensated_run(ctx, prev, curr, mv, nullptr, kind, outs, factors, count, match_sad, name, nullptr, 0, sampling);
}

}  // namespace

LFG_EXPORT int lfg_interpolate_compensated_sampled(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                                   lfg_frame *out, float factor, int match_sad, int sampling) {
    lfg_frame *const outs[1] = {out};
    return compensated_sampled(ctx, prev, curr, mv, outs, &factor, 1, match_sad, sampling, "lfg_interpolate_compensated_sampled");
}

LFG_EXPORT int lfg_interpolate_compensated_sampled_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                                         lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad,
                                                         int sampling) {
    return compensated_sampled(ctx, prev, curr, mv, outs, factors, count, match_sad, sampling, "lfg_interpolate_compensated_sampled_multi");
}

LFG_EXPORT int lfg_set_sampling(lfg_context *ctx, int sampling) {
    if (!ctx) return LFG_ERR_INVALID;
    if (sampling != LFG_SAMPLING_BILINEAR && sampling != LFG_SAMPLING_BICUBIC)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_sampling: sampling must be LFG_SAMPLING_BILINEAR or LFG_SAMPLING_BICUBIC");
    ctx->sampling = sampling;
    return LFG_OK;
}

LFG_EXPORT int lfg_sampling_effective(const lfg_context *ctx) {
    return ctx ? sampling_effective(ctx) : (int)LFG_SAMPLING_BILINEAR;
}

// ---- scene-cut detection (pair_stats.hip)

LFG_EXPORT int lfg_pair_match(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                              int match_sad, void *device_stats) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(mv, LFG_FORMAT_MV_S8X2))
        return fail(ctx, LFG_ERR_INVALID, "lfg_pair_match: prev/curr must be RGBA8 and mv MV_S8X2, all non-empty");
    if (!same_size(prev, curr) || !same_size(curr, mv))
        return fail(ctx, LFG_ERR_INVALID, "lfg_pair_match: prev, curr and mv differ in size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u || mv->pitch % 2u || (uintptr_t)mv->data % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_pair_match: RGBA8 frames must be 4-byte aligned and mv 2-byte aligned");
    if (match_sad < 0 || match_sad > 1020) return fail(ctx, LFG_ERR_INVALID, "lfg_pair_match: match_sad must be in [0, 1020]");
    if (!device_stats || (uintptr_t)device_stats % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_pair_match: device_stats must be non-NULL and 8-byte aligned");
    StageTimer timer(ctx, LFG_STAGE_MOTION);
    hipError_t e = lfg::launch_pair_match(ctx->cur().stream, *prev, *curr, *mv, match_sad, ctx->device_cus, device_stats);
    if (e != hipSuccess) return fail_hip(ctx, e, "pair match kernel launch");
    return LFG_OK;
}

namespace {

int cut_fallback_check(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const void *device_stats,
                       int min_matched_permille, lfg_frame *const *outs, const float *factors, uint32_t count) {
    if (!outs || !factors || count == 0 || count > LFG_MAX_FACTORS)
        return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: count must be in [1, LFG_MAX_FACTORS] and outs/factors non-NULL");
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: prev/curr must be non-empty RGBA8");
    if (!same_size(prev, curr)) return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: prev and curr differ in size");
    if ((prev->pitch | curr->pitch) % 4u || ((uintptr_t)prev->data | (uintptr_t)curr->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: RGBA8 frames must be 4-byte aligned");
    if (!device_stats || (uintptr_t)device_stats % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: device_stats must be non-NULL and 8-byte aligned");
    if (min_matched_permille < 0 || min_matched_permille > 1000)
        return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: min_matched_permille must be in [0, 1000]");
    for (uint32_t i = 0; i < count; ++i) {
        const lfg_frame *o = outs[i];
        if (!frame_ok(o, LFG_FORMAT_RGBA8_UNORM) || !same_size(curr, o) || o->pitch % 4u || (uintptr_t)o->data % 4u)
            return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: bad output frame (NULL, empty, wrong format, size or alignment)");
        if (frames_overlap(o, prev) || frames_overlap(o, curr))
            return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: an output overlaps an input");
        for (uint32_t j = 0; j < i; ++j)
            if (frames_overlap(outs[j], o)) return fail(ctx, LFG_ERR_INVALID, "lfg_cut_fallback: two outputs overlap each other");
    }
    return LFG_OK;
}

int cut_fallback_enqueue(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const void *device_stats,
                         int min_matched_permille, lfg_frame *const *outs, const float *factors, uint32_t count) {
    StageTimer timer(ctx, LFG_STAGE_INTERPOLATE);
    hipError_t e = lfg::launch_cut_fallback(ctx->cur().stream, *prev, *curr, device_stats, min_matched_permille, outs, factors,
                                            (int)count, ctx->device_cus);
    if (e != hipSuccess) return fail_hip(ctx, e, "cut fallback kernel launch");
    return LFG_OK;
}

}  // namespace

LFG_EXPORT int lfg_cut_fallback(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const void *device_stats,
                                int min_matched_permille, lfg_frame *const *outs, const float *factors, uint32_t count) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = cut_fallback_check(ctx, prev, curr, device_stats, min_matched_permille, outs, factors, count);
    if (rc != LFG_OK) return rc;
    return cut_fallback_enqueue(ctx, prev, curr, device_stats, min_matched_permille, outs, factors, count);
}

LFG_EXPORT int lfg_set_cut_detection(lfg_context *ctx, int min_matched_permille) {
    if (!ctx) return LFG_ERR_INVALID;
    if (min_matched_permille < -1 || min_matched_permille > 1000)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_cut_detection: min_matched_permille must be -1 (off) or in [0, 1000]");
    ctx->cut_permille = min_matched_permille;
    return LFG_OK;
}

LFG_EXPORT int lfg_last_pair_stats(lfg_context *ctx, lfg_pair_stats *out_stats, int *out_cut) {
    if (!ctx) return LFG_ERR_INVALID;
    const lfg::CutDetectState &cut = ctx->cur().cut;
    if (!cut.recorded) return fail(ctx, LFG_ERR_INVALID, "lfg_last_pair_stats: the selected lane has made no call with cut detection on");
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    LFG_HIP(ctx, hipEventSynchronize(cut.event));
    const lfg_pair_stats s = *cut.pinned;
    if (out_stats) *out_stats = s;
    if (out_cut) *out_cut = s.matched * 1000ull < (uint64_t)cut.permille * s.pixels ? 1 : 0;
    return LFG_OK;
}

// ---- frame comparison (frame_diff.hip)

LFG_EXPORT int lfg_frame_diff(lfg_context *ctx, const lfg_frame *a, const lfg_frame *b, uint32_t channel_mask,
                              int accumulate, void *device_stats) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(a, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(b, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_diff: a and b must be non-empty RGBA8");
    if (!same_size(a, b)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_diff: a and b differ in size");
    if ((a->pitch | b->pitch) % 4u || ((uintptr_t)a->data | (uintptr_t)b->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_diff: RGBA8 frames must be 4-byte aligned");
    if (channel_mask < 1u || channel_mask > 15u) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_diff: channel_mask must be in [1, 15]");
    if (accumulate != 0 && accumulate != 1) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_diff: accumulate must be 0 or 1");
    if (!device_stats || (uintptr_t)device_stats % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_diff: device_stats must be non-NULL and 8-byte aligned");
    hipError_t e = lfg::launch_frame_diff(ctx->cur().stream, *a, *b, channel_mask, accumulate == 1, ctx->device_cus, device_stats);
    if (e != hipSuccess) return fail_hip(ctx, e, "frame diff kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_frame_diff_summarize(const lfg_frame_diff_stats *host_stats, uint32_t channel_mask, lfg_frame_diff_summary *out) {
    if (!host_stats || !out || channel_mask < 1u || channel_mask > 15u || host_stats->pixels == 0) return LFG_ERR_INVALID;
    const uint64_t pixels = host_stats->pixels;
    uint64_t total = 0;
    for (int k = 0; k < 256; ++k) {
        if (host_stats->hist[k] > pixels - total) return LFG_ERR_INVALID;       // (no sum past pixels: no wrap either)
        total += host_stats->hist[k];
    }
    if (total != pixels) return LFG_ERR_INVALID;
    lfg_frame_diff_summary s{};
    s.pixels = pixels;
    s.differing = pixels - host_stats->hist[0];
    s.over_1 = s.differing - host_stats->hist[1];
    // the quantiles: 100 * below >= P * pixels.  64 bits hold both products for any record the device can have written
    // (pixels below 2^57); a hand-made record may be larger, hence the wider type
    bool have50 = false, have99 = false;
    uint64_t below = 0;
    for (uint32_t k = 0; k < 256u; ++k) {
        below += host_stats->hist[k];
        if (host_stats->hist[k] > 0) s.max_abs = k;
        const unsigned __int128 lhs = (unsigned __int128)100u * below;
        if (!have50 && lhs >= (unsigned __int128)50u * pixels) { s.p50 = k; have50 = true; }
        if (!have99 && lhs >= (unsigned __int128)99u * pixels) { s.p99 = k; have99 = true; }
    }
    double sum = 0.0;
    int channels = 0;
    for (int c = 0; c < 4; ++c)
        if ((channel_mask >> c) & 1u) { sum += (double)host_stats->sse[c]; ++channels; }
    s.mse = sum / ((double)channels * (double)pixels);
    s.psnr_db = s.mse > 0.0 ? 10.0 * std::log10(65025.0 / s.mse) : HUGE_VAL;
    *out = s;
    return LFG_OK;
}

// ---- level matching (levels.hip)

static_assert(sizeof(lfg_frame_histogram_stats) == lfg::kHistWords * 8 && sizeof(lfg_levels_map) == lfg::kMapBytes &&
              offsetof(lfg_levels_map, forward) == lfg::kMapHeadBytes, "lfg_levels.hpp lays the records out as the header declares them");

LFG_EXPORT int lfg_frame_histogram(lfg_context *ctx, const lfg_frame *frame, int accumulate, void *device_stats) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(frame, LFG_FORMAT_RGBA8_UNORM)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_histogram: frame must be non-empty RGBA8");
    if (frame->pitch % 4u || (uintptr_t)frame->data % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_histogram: RGBA8 frames must be 4-byte aligned");
    if (accumulate != 0 && accumulate != 1) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_histogram: accumulate must be 0 or 1");
    if (!device_stats || (uintptr_t)device_stats % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_histogram: device_stats must be non-NULL and 8-byte aligned");
    hipError_t e = lfg::launch_frame_histogram(ctx->cur().stream, *frame, accumulate == 1, ctx->device_cus, device_stats);
    if (e != hipSuccess) return fail_hip(ctx, e, "frame histogram kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_levels_match(lfg_context *ctx, const void *device_hist_from, const void *device_hist_to, int min_shift16,
                                void *device_map) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!device_hist_from || !device_hist_to || !device_map ||
        ((uintptr_t)device_hist_from | (uintptr_t)device_hist_to | (uintptr_t)device_map) % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_match: both records and the map must be non-NULL and 8-byte aligned");
    if (min_shift16 < 0 || min_shift16 > lfg::kLevelsMaxShift16)
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_match: min_shift16 must be in [0, 4080]");
    const uintptr_t m0 = (uintptr_t)device_map, m1 = m0 + sizeof(lfg_levels_map);
    for (const void *h : {device_hist_from, device_hist_to})
        if ((uintptr_t)h < m1 && m0 < (uintptr_t)h + sizeof(lfg_frame_histogram_stats))
            return fail(ctx, LFG_ERR_INVALID, "lfg_levels_match: the map overlaps a record");
    hipError_t e = lfg::launch_levels_match(ctx->cur().stream, device_hist_from, device_hist_to, min_shift16, device_map);
    if (e != hipSuccess) return fail_hip(ctx, e, "levels match kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_levels_apply(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, const void *device_map, int mode, float factor) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(in, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: in and out must be non-empty RGBA8");
    if (!same_size(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: in and out differ in size");
    if ((in->pitch | out->pitch) % 4u || ((uintptr_t)in->data | (uintptr_t)out->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: RGBA8 frames must be 4-byte aligned");
    if (!(in->data == out->data && in->pitch == out->pitch) && frames_overlap(in, out))
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: out overlaps in without being in itself");
    if (!device_map || (uintptr_t)device_map % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: device_map must be non-NULL and 8-byte aligned");
    if (mode != LFG_LEVELS_FORWARD && mode != LFG_LEVELS_AT) return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: mode must be LFG_LEVELS_FORWARD or LFG_LEVELS_AT");
    if (mode == LFG_LEVELS_AT && (!std::isfinite(factor) || factor < 0.0f || factor > 1.0f))
        return fail(ctx, LFG_ERR_INVALID, "lfg_levels_apply: under LFG_LEVELS_AT the factor must be a finite number in [0, 1]");
    const int tq = mode == LFG_LEVELS_AT ? lfg::levels_tq(factor) : 0;
    hipError_t e = lfg::launch_levels_apply(ctx->cur().stream, *in, *out, device_map, mode, tq);
    if (e != hipSuccess) return fail_hip(ctx, e, "levels apply kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_level_matching(lfg_context *ctx, int min_shift16) {
    if (!ctx) return LFG_ERR_INVALID;
    if (min_shift16 < -1 || min_shift16 > lfg::kLevelsMaxShift16)
        return fail(ctx, LFG_ERR_INVALID, "lfg_set_level_matching: min_shift16 must be -1 (off) or in [0, 4080]");
    ctx->level_shift16 = min_shift16;
    return LFG_OK;
}

LFG_EXPORT int lfg_last_level_match(lfg_context *ctx, uint64_t *out_shift_sum, uint64_t *out_pixels, int *out_active) {
    if (!ctx) return LFG_ERR_INVALID;
    const lfg::LevelMatchState &lv = ctx->cur().levels;
    if (!lv.recorded) return fail(ctx, LFG_ERR_INVALID, "lfg_last_level_match: the selected lane has made no call with level matching on");
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    LFG_HIP(ctx, hipEventSynchronize(lv.event));
    if (out_pixels) *out_pixels = lv.pinned[0];
    if (out_shift_sum) *out_shift_sum = lv.pinned[1];
    if (out_active) *out_active = (uint32_t)lv.pinned[2] != 0u ? 1 : 0;
    return LFG_OK;
}

// ---- structural similarity (frame_ssim.hip)

LFG_EXPORT int lfg_frame_ssim(lfg_context *ctx, const lfg_frame *a, const lfg_frame *b, uint32_t channel_mask,
                              int accumulate, void *device_stats) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(a, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(b, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: a and b must be non-empty RGBA8");
    if (!same_size(a, b)) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: a and b differ in size");
    if (a->width < 8u || a->height < 8u || a->width > 262144u || a->height > 262144u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: width and height must be in [8, 262144]");
    if ((a->pitch | b->pitch) % 4u || ((uintptr_t)a->data | (uintptr_t)b->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: RGBA8 frames must be 4-byte aligned");
    if (channel_mask < 1u || channel_mask > 15u) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: channel_mask must be in [1, 15]");
    if (accumulate != 0 && accumulate != 1) return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: accumulate must be 0 or 1");
    if (!device_stats || (uintptr_t)device_stats % 8u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_frame_ssim: device_stats must be non-NULL and 8-byte aligned");
    hipError_t e = lfg::launch_frame_ssim(ctx->cur().stream, *a, *b, channel_mask, accumulate == 1, ctx->device_cus, device_stats);
    if (e != hipSuccess) return fail_hip(ctx, e, "frame ssim kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_frame_ssim_summarize(const lfg_frame_ssim_stats *host_stats, uint32_t channel_mask, lfg_frame_ssim_summary *out) {
    if (!host_stats || !out || channel_mask < 1u || channel_mask > 15u || host_stats->windows == 0) return LFG_ERR_INVALID;
    const uint64_t windows = host_stats->windows;
    uint64_t total = 0, below = 0;
    for (int k = 0; k < 65; ++k) {
        if (host_stats->hist[k] > windows - total) return LFG_ERR_INVALID;      // (no sum past windows: no wrap either)
        total += host_stats->hist[k];
        if (k < 32) below += host_stats->hist[k];
    }
    if (total != windows) return LFG_ERR_INVALID;
    lfg_frame_ssim_summary s{};
    s.windows = windows;
    s.identical = host_stats->hist[64];
    s.below_half = below;
    const double scale = (double)windows * 16777216.0;
    double sum = 0.0;
    int channels = 0;
    for (int c = 0; c < 4; ++c) {
        s.ssim[c] = (double)host_stats->sum[c] / scale;
        if ((channel_mask >> c) & 1u) { sum += s.ssim[c]; ++channels; }
    }
    s.all = sum / (double)channels;
    s.db = s.all < 1.0 ? -10.0 * std::log10(1.0 - s.all) : HUGE_VAL;
    s.worst_value = ((double)(host_stats->worst >> 32) - 16777216.0) / 16777216.0;
    s.worst_x = 4u * (uint32_t)(host_stats->worst & 0xffffu);
    s.worst_y = 4u * (uint32_t)((host_stats->worst >> 16) & 0xffffu);
    *out = s;
    return LFG_OK;
}

// ---- colour conversion (yuv_convert.hip)

LFG_EXPORT int lfg_yuv_coefficients(int matrix, int range, int32_t to_rgb[5], int32_t to_yuv[9]) {
    if (!to_rgb || !to_yuv || (matrix != LFG_YUV_BT601 && matrix != LFG_YUV_BT709) || (range != LFG_YUV_LIMITED && range != LFG_YUV_FULL))
        return LFG_ERR_INVALID;
    const double kr = matrix == LFG_YUV_BT601 ? 0.299 : 0.2126, kb = matrix == LFG_YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double sy = range == LFG_YUV_LIMITED ? 255.0 / 219.0 : 1.0, sc = range == LFG_YUV_LIMITED ? 255.0 / 224.0 : 1.0;
    const auto q14 = [](double x) { return (int32_t)std::llround(x * 16384.0); };        // (none is a tie: tests/yuv_model.py)
    to_rgb[0] = q14(sy);
    to_rgb[1] = q14(2.0 * (1.0 - kr) * sc);
    to_rgb[2] = q14(2.0 * kb * (1.0 - kb) / kg * sc);
    to_rgb[3] = q14(2.0 * kr * (1.0 - kr) / kg * sc);
    to_rgb[4] = q14(2.0 * (1.0 - kb) * sc);
    to_yuv[0] = q14(kr / sy);
    to_yuv[2] = q14(kb / sy);
    to_yuv[1] = q14(1.0 / sy) - to_yuv[0] - to_yuv[2];
    to_yuv[3] = q14(-kr / (2.0 * (1.0 - kb)) / sc);
    to_yuv[5] = q14(0.5 / sc);
    to_yuv[4] = -to_yuv[3] - to_yuv[5];
    to_yuv[6] = q14(0.5 / sc);
    to_yuv[8] = q14(-kb / (2.0 * (1.0 - kr)) / sc);
    to_yuv[7] = -to_yuv[6] - to_yuv[8];
    return LFG_OK;
}

namespace {

// The bytes a plane or a frame spans, for the overlap rules.
struct Span { uintptr_t lo, hi; };
Span span_of(const void *base, uint32_t pitch, uint32_t rows, size_t rowBytes) {
    return Span{(uintptr_t)base, (uintptr_t)base + (size_t)pitch * (rows - 1u) + rowBytes};
}
bool spans_overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }

// Everything lfg_nv12_to_rgba and lfg_rgba_to_nv12 require; fills `k`.  `planesOut`: the planes are the output.
int yuv_check(lfg_context *ctx, const lfg_nv12 *p, const lfg_frame *f, int matrix, int range, int siting, bool planesOut,
              const char *name, lfg::YuvCoefficients &k) {
    const std::string n = name;
    if (!p || !p->y || !p->uv || !frame_ok(f, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, n + ": NULL pointer, or the RGBA frame is empty or of another format");
    if (p->width == 0 || p->height == 0 || p->width % 2u || p->height % 2u || p->width != f->width || p->height != f->height)
        return fail(ctx, LFG_ERR_INVALID, n + ": width and height must be even, non-zero and equal to the RGBA frame's");
    if (p->y_pitch < p->width || p->uv_pitch < p->width || p->uv_pitch % 2u || (uintptr_t)p->uv % 2u)
        return fail(ctx, LFG_ERR_INVALID, n + ": y_pitch and uv_pitch must be at least the width, uv_pitch even and uv 2-byte aligned");
    if (f->pitch % 4u || (uintptr_t)f->data % 4u)
        return fail(ctx, LFG_ERR_INVALID, n + ": the RGBA frame must be 4-byte aligned with a pitch that is a multiple of 4");
    if (siting != LFG_CHROMA_REPLICATE && siting != LFG_CHROMA_LEFT) return fail(ctx, LFG_ERR_INVALID, n + ": unknown chroma siting");
    if (lfg_yuv_coefficients(matrix, range, k.to_rgb, k.to_yuv) != LFG_OK) return fail(ctx, LFG_ERR_INVALID, n + ": unknown matrix or range");
    k.offset = range == LFG_YUV_LIMITED ? 16 : 0;
    const Span y = span_of(p->y, p->y_pitch, p->height, p->width), uv = span_of(p->uv, p->uv_pitch, p->height / 2u, p->width);
    const Span rgba = span_of(f->data, f->pitch, f->height, (size_t)f->width * 4u);
    if (spans_overlap(y, rgba) || spans_overlap(uv, rgba)) return fail(ctx, LFG_ERR_INVALID, n + ": the output overlaps an input");
    if (planesOut && spans_overlap(y, uv)) return fail(ctx, LFG_ERR_INVALID, n + ": the two output planes overlap each other");
    if (!lfg::yuv_grid_ok(p->width, p->height)) return fail(ctx, LFG_ERR_INVALID, n + ": frame larger than 8,388,480 x 524,280");
    return LFG_OK;
}

}  // namespace

LFG_EXPORT int lfg_nv12_to_rgba(lfg_context *ctx, const lfg_nv12 *in, lfg_frame *out, int matrix, int range, int siting) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    lfg::YuvCoefficients k;
    const int rc = yuv_check(ctx, in, out, matrix, range, siting, false, "lfg_nv12_to_rgba", k);
    if (rc != LFG_OK) return rc;
    hipError_t e = lfg::launch_nv12_to_rgba(ctx->cur().stream, *in, *out, k, siting);
    if (e != hipSuccess) return fail_hip(ctx, e, "NV12 to RGBA kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_rgba_to_nv12(lfg_context *ctx, const lfg_frame *in, const lfg_nv12 *out, int matrix, int range, int siting) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    lfg::YuvCoefficients k;
    const int rc = yuv_check(ctx, out, in, matrix, range, siting, true, "lfg_rgba_to_nv12", k);
    if (rc != LFG_OK) return rc;
    hipError_t e = lfg::launch_rgba_to_nv12(ctx->cur().stream, *in, *out, k, siting);
    if (e != hipSuccess) return fail_hip(ctx, e, "RGBA to NV12 kernel launch");
    return LFG_OK;
}

// ---- sharpening of presented frames (sharpen.hip)

LFG_EXPORT int lfg_sharpen(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int strength) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(in, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_sharpen: in and out must be non-empty RGBA8");
    if (!same_size(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_sharpen: in and out differ in size");
    if ((in->pitch | out->pitch) % 4u || ((uintptr_t)in->data | (uintptr_t)out->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_sharpen: RGBA8 frames must be 4-byte aligned with a pitch that is a multiple of 4");
    if (strength < 0 || strength > 64) return fail(ctx, LFG_ERR_INVALID, "lfg_sharpen: strength must be in [0, 64]");
    if (frames_overlap(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_sharpen: the output overlaps the input");
    hipError_t e = lfg::launch_sharpen(ctx->cur().stream, *in, *out, strength);
    if (e != hipSuccess) return fail_hip(ctx, e, "sharpen kernel launch");
    return LFG_OK;
}

// ---- debanding with dithered output of presented frames (deband.hip)

LFG_EXPORT int lfg_deband(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int iterations, int threshold, int radius, int grain,
                          uint32_t seed) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(in, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_deband: in and out must be non-empty RGBA8");
    if (!same_size(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_deband: in and out differ in size");
    if ((in->pitch | out->pitch) % 4u || ((uintptr_t)in->data | (uintptr_t)out->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_deband: RGBA8 frames must be 4-byte aligned with a pitch that is a multiple of 4");
    if (iterations < 1 || iterations > lfg::kDebandMaxIterations) return fail(ctx, LFG_ERR_INVALID, "lfg_deband: iterations must be in [1, 4]");
    if (threshold < 0 || threshold > lfg::kDebandMaxThreshold) return fail(ctx, LFG_ERR_INVALID, "lfg_deband: threshold must be in [0, 64]");
    if (radius < 1 || radius > lfg::kDebandMaxRadius) return fail(ctx, LFG_ERR_INVALID, "lfg_deband: radius must be in [1, 32]");
    if (grain < 0 || grain > lfg::kDebandMaxGrain) return fail(ctx, LFG_ERR_INVALID, "lfg_deband: grain must be in [0, 16]");
    if (frames_overlap(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_deband: the output overlaps the input");
    hipError_t e = lfg::launch_deband(ctx->cur().stream, *in, *out, iterations, threshold, radius, grain, seed);
    if (e != hipSuccess) return fail_hip(ctx, e, "deband kernel launch");
    return LFG_OK;
}

// The draw of one pixel, through the functions the kernel draws with (lfg_deband.hpp).
LFG_EXPORT int lfg_deband_draw(uint32_t seed, uint32_t x, uint32_t y, int iterations, int radius, int32_t offsets[8], int32_t noise_bytes[3]) {
    if (!offsets || !noise_bytes || iterations < 1 || iterations > lfg::kDebandMaxIterations || radius < 1 || radius > lfg::kDebandMaxRadius)
        return LFG_ERR_INVALID;
    const uint32_t r0 = lfg::deband_r0(lfg::deband_row_key(lfg::deband_seed_key(seed), y), x);
    for (int i = 0; i < lfg::kDebandMaxIterations; ++i) {
        const lfg::DebandOffset o = i < iterations ? lfg::deband_offset(lfg::deband_r(r0, (uint32_t)(i + 1)), radius * (i + 1)) : lfg::DebandOffset{0, 0};
        offsets[2 * i] = o.x;
        offsets[2 * i + 1] = o.y;
    }
    const uint32_t noise = lfg::deband_r(r0, lfg::kDebandNoiseDraw);
    for (int c = 0; c < 3; ++c) noise_bytes[c] = (int32_t)((noise >> (8 * c)) & 255u);
    return LFG_OK;
}

// ---- motion-compensated temporal denoising (denoise.hip)

LFG_EXPORT int lfg_denoise_temporal(lfg_context *ctx, const lfg_frame *curr, const lfg_frame *const *refs, const lfg_frame *const *mvs,
                                    int count, lfg_frame *out, int radius, int tolerance, int strength, int limit) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (count < 1 || count > lfg::kDenoiseMaxRefs) return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: count must be 1 or 2");
    if (!refs || !mvs) return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: refs and mvs must not be NULL");
    if (!frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: curr and out must be non-empty RGBA8");
    if (!same_size(curr, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: curr and out differ in size");
    if ((curr->pitch | out->pitch) % 4u || ((uintptr_t)curr->data | (uintptr_t)out->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: RGBA8 frames must be 4-byte aligned with a pitch that is a multiple of 4");
    if (frames_overlap(out, curr)) return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: out overlaps curr (it cannot run in place)");
    for (int i = 0; i < count; ++i) {
        if (mvs[i] && mvs[i]->format == LFG_FORMAT_MV_S16X2_Q2)
            return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: quarter-pixel vectors (MV_S16X2_Q2) are not supported");
        if (!frame_ok(refs[i], LFG_FORMAT_RGBA8_UNORM) || !frame_ok(mvs[i], LFG_FORMAT_MV_S8X2))
            return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: every reference must be non-empty RGBA8 and every field MV_S8X2");
        if (!same_size(curr, refs[i]) || !same_size(curr, mvs[i]))
            return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: curr, the references and the fields differ in size");
        if (refs[i]->pitch % 4u || (uintptr_t)refs[i]->data % 4u)
            return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: RGBA8 frames must be 4-byte aligned with a pitch that is a multiple of 4");
        if (mvs[i]->pitch % 2u || (uintptr_t)mvs[i]->data % 2u)
            return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: mv must be 2-byte aligned with a pitch that is a multiple of 2");
        if (frames_overlap(out, refs[i]) || frames_overlap(out, mvs[i]))
            return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: out overlaps a reference or a field");
    }
    if (radius < 0 || radius > lfg::kDenoiseMaxRadius) return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: radius must be in [0, 2]");
    if (tolerance < 1 || tolerance > lfg::kDenoiseMaxTolerance)
        return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: tolerance must be in [1, 1020]");
    if (strength < 0 || strength > lfg::kDenoiseMaxStrength)
        return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: strength must be in [0, 256]");
    if (limit < 0 || limit > lfg::kDenoiseMaxLimit) return fail(ctx, LFG_ERR_INVALID, "lfg_denoise_temporal: limit must be in [0, 255]");
    hipError_t e = lfg::launch_denoise_temporal(ctx->cur().stream, *curr, refs, mvs, count, *out, radius, tolerance, strength, limit);
    if (e != hipSuccess) return fail_hip(ctx, e, "temporal denoise kernel launch");
    return LFG_OK;
}

// ---- resampling with a choice of filter (resample.hip)

namespace {

// The cubic of Mitchell and Netravali; |x| < 2.
double resample_cubic(double x, double B, double C) {
    x = std::fabs(x);
    if (x < 1.0) return ((12.0 - 9.0 * B - 6.0 * C) * x * x * x + (-18.0 + 12.0 * B + 6.0 * C) * x * x + (6.0 - 2.0 * B)) / 6.0;
    if (x < 2.0) return ((-B - 6.0 * C) * x * x * x + (6.0 * B + 30.0 * C) * x * x + (-12.0 * B - 48.0 * C) * x + (8.0 * B + 24.0 * C)) / 6.0;
    return 0.0;
}

double resample_lanczos(double x, double a) {
    if (x == 0.0) return 1.0;
    if (std::fabs(x) >= a) return 0.0;
    const double px = 3.141592653589793238462643383279502884 * x;
    return a * std::sin(px) * std::sin(px / a) / (px * px);
}

double resample_filter(int filter, double x) {
    switch (filter) {
        case LFG_FILTER_BILINEAR: return std::fabs(x) < 1.0 ? 1.0 - std::fabs(x) : 0.0;
        case LFG_FILTER_CATMULL_ROM: return resample_cubic(x, 0.0, 0.5);
        case LFG_FILTER_MITCHELL: return resample_cubic(x, 1.0 / 3.0, 1.0 / 3.0);
        case LFG_FILTER_LANCZOS2: return resample_lanczos(x, 2.0);
        default: return resample_lanczos(x, 3.0);
    }
}

int resample_support(int filter) { return filter == LFG_FILTER_BILINEAR ? 1 : filter == LFG_FILTER_LANCZOS3 ? 3 : 2; }

bool resample_filter_known(int filter) { return filter >= LFG_FILTER_NEAREST && filter <= LFG_FILTER_LANCZOS3; }

__int128 floor_div(__int128 a, __int128 b) {                 // b > 0
    const __int128 q = a / b;
    return a % b != 0 && a < 0 ? q - 1 : q;
}

}  // namespace

LFG_EXPORT int lfg_resample_taps(int filter, uint32_t in_size, uint32_t out_size, int32_t *first, uint32_t *count, int16_t *weights) {
    if (!first || !count || !weights || in_size == 0 || out_size == 0 || in_size > 0x7fffffffu || !resample_filter_known(filter))
        return LFG_ERR_INVALID;
    constexpr int kMax = LFG_RESAMPLE_MAX_TAPS;
    const __int128 in = in_size, out = out_size, D = 2 * (in > out ? in : out), lim = resample_support(filter) * D;
    for (uint32_t p = 0; p < out_size; ++p) {
        int16_t *row = weights + (size_t)p * kMax;
        for (int j = 0; j < kMax; ++j) row[j] = 0;
        const __int128 centre = (2 * (__int128)p + 1) * in;
        if (filter == LFG_FILTER_NEAREST) {
            first[p] = (int32_t)floor_div(centre, 2 * out);
            count[p] = 1u;
            row[0] = 16384;
            continue;
        }
        // the integers k with |(2k + 1) out - centre| < lim
        const __int128 k0 = floor_div(centre - lim - out, 2 * out) + 1;
        const __int128 k1 = floor_div(centre + lim - out + 2 * out - 1, 2 * out) - 1;
        const __int128 taps = k1 - k0 + 1;
        if (taps > kMax) return LFG_ERR_UNSUPPORTED;
        const int n = (int)taps;
        double raw[kMax], sum = 0.0;
        for (int j = 0; j < n; ++j) {
            raw[j] = resample_filter(filter, (double)((2 * (k0 + j) + 1) * out - centre) / (double)D);
            sum += raw[j];
        }
        const auto clamped = [&](__int128 k) { return k < 0 ? (__int128)0 : k > in - 1 ? in - 1 : k; };
        const __int128 lo = clamped(k0);
        const int span = (int)(clamped(k1) - lo) + 1;
        double folded[kMax];
        for (int j = 0; j < span; ++j) folded[j] = 0.0;
        for (int j = 0; j < n; ++j) folded[(int)(clamped(k0 + j) - lo)] += raw[j] / sum;
        long q[kMax], total = 0, magnitude = 0;
        int big = 0;
        for (int j = 0; j < span; ++j) {
            q[j] = std::lrint(folded[j] * 16384.0);           // (ties to even: the default rounding mode)
            total += q[j];
            if (std::labs(q[j]) > std::labs(q[big])) big = j;
        }
        q[big] += 16384 - total;
        for (int j = 0; j < span; ++j) magnitude += std::labs(q[j]);
        if (magnitude > 32768) return LFG_ERR_UNSUPPORTED;
        first[p] = (int32_t)lo;
        count[p] = (uint32_t)span;
        for (int j = 0; j < span; ++j) row[j] = (int16_t)q[j];
    }
    return LFG_OK;
}

LFG_EXPORT int lfg_light_tables(int light, uint16_t *forward, uint16_t *threshold) {
    if (!forward || !threshold || (light != LFG_LIGHT_LINEAR && light != LFG_LIGHT_SIGMOID)) return LFG_ERR_INVALID;
    constexpr double kCentre = 0.75, kSlope = 6.5;              // the sigmoid of mpv and libplacebo
    const double offset = 1.0 / (1.0 + std::exp(kSlope * kCentre));
    const double scale = 1.0 / (1.0 + std::exp(kSlope * (kCentre - 1.0))) - offset;
    for (int b = 0; b < 256; ++b) {
        const double c = (double)b / 255.0;
        double f = c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
        if (light == LFG_LIGHT_SIGMOID) f = kCentre - std::log(1.0 / (f * scale + offset) - 1.0) / kSlope;
        forward[b] = (uint16_t)std::floor(16383.0 * f + 0.5);
    }
    for (int k = 1; k < 256; ++k) threshold[k - 1] = (uint16_t)(((uint32_t)forward[k - 1] + (uint32_t)forward[k] + 1u) >> 1);
    return LFG_OK;
}

LFG_EXPORT int lfg_resample_brackets(uint32_t in_size, uint32_t out_size, int32_t *lo, int32_t *hi) {
    if (!lo || !hi || in_size == 0 || out_size == 0 || in_size > 0x7fffffffu) return LFG_ERR_INVALID;
    const __int128 in = in_size, out = out_size, D = 2 * out;
    const auto clamped = [&](__int128 k) { return k < 0 ? (__int128)0 : k > in - 1 ? in - 1 : k; };
    for (uint32_t p = 0; p < out_size; ++p) {
        const __int128 N = (2 * (__int128)p + 1) * in - out;
        lo[p] = (int32_t)clamped(floor_div(N, D));
        hi[p] = (int32_t)clamped(-floor_div(-N, D));           // the ceiling: lo where the centre is a texel's
    }
    return LFG_OK;
}

namespace {

// The brackets of one growing axis (out > in), built and uploaded at their first use.  The kernel reads texel a(p) and b(p) of
// a row, and LDS row a(q) and b(q) of a tile, without a check of its own, on the strength of the lemma
//   first[p] <= a(p) <= b(p) < first[p] + count[p]   for every filter of support >= 1,
// which is asserted here on the taps of support 1, |(2k + 1) out - (2p + 1) in| < 2 out folded onto 0 .. in - 1: a wider
// filter's taps hold those, and folding is monotone.
int resample_bracket_table(lfg_context *ctx, uint32_t in_size, uint32_t out_size, lfg::ResampleBracket *out) {
    if (const auto hit = ctx->resample_brackets.find(std::make_pair(in_size, out_size))) { *out = hit->bracket; return LFG_OK; }
    const size_t n = out_size;
    std::vector<int32_t> host(2 * n);
    if (lfg_resample_brackets(in_size, out_size, host.data(), host.data() + n) != LFG_OK)
        return fail(ctx, LFG_ERR_INVALID, "lfg_resample_antiring: a frame of this size has no brackets");
    const __int128 in = in_size, o = out_size;
    for (size_t p = 0; p < n; ++p) {
        const __int128 centre = (2 * (__int128)p + 1) * in;
        const __int128 k0 = floor_div(centre - 3 * o, 2 * o) + 1, k1 = floor_div(centre + 3 * o - 1, 2 * o) - 1;
        const auto clamped = [&](__int128 k) { return k < 0 ? (__int128)0 : k > in - 1 ? in - 1 : k; };
        const __int128 first = clamped(k0), last = clamped(k1);
        if (!(first <= host[p] && host[p] <= host[n + p] && host[n + p] <= last))
            return fail(ctx, LFG_ERR_INVALID, "lfg_resample_antiring: a bracket outside its taps (" + std::to_string(in_size) + " -> " +
                                                  std::to_string(out_size) + ", sample " + std::to_string(p) + ")");
    }
    lfg::ResampleBracketTable t;
    t.in_size = in_size; t.out_size = out_size;
    const int rc = upload_table(ctx, host.data(), 2 * n * sizeof(int32_t), "resample brackets", &t.d_base);
    if (rc != LFG_OK) return rc;
    t.bracket.lo = reinterpret_cast<int32_t *>(t.d_base);
    t.bracket.hi = t.bracket.lo + n;
    ctx->resample_brackets.insert(t);
    *out = t.bracket;
    return LFG_OK;
}

// The table of one axis, built and uploaded at its first use.  Returned by value: the pointers in it are the device's.
int resample_table(lfg_context *ctx, int filter, uint32_t in_size, uint32_t out_size, lfg::ResampleTable *out) {
    if (const auto hit = ctx->resample_tables.find(std::make_tuple(filter, in_size, out_size))) { *out = *hit; return LFG_OK; }
    const size_t n = out_size;
    std::vector<int32_t> first(n);
    std::vector<uint32_t> count(n);
    std::vector<int16_t> weights(n * LFG_RESAMPLE_MAX_TAPS);
    const int rc = lfg_resample_taps(filter, in_size, out_size, first.data(), count.data(), weights.data());
    if (rc == LFG_ERR_UNSUPPORTED)
        return fail(ctx, rc, "lfg_resample: " + std::to_string(in_size) + " -> " + std::to_string(out_size) +
                                 " needs more than LFG_RESAMPLE_MAX_TAPS taps per sample under this filter");
    if (rc != LFG_OK) return fail(ctx, rc, "lfg_resample: a frame of this size has no table");
    lfg::ResampleTable t;
    t.filter = filter; t.in_size = in_size; t.out_size = out_size;
    t.plan = lfg::resample_plan(first.data(), count.data(), out_size);
    // the device's rows are as long as the longest row here, rounded up to even, instead of LFG_RESAMPLE_MAX_TAPS
    uint32_t stride = 2;
    for (size_t p = 0; p < n; ++p) stride = std::max(stride, (count[p] + 1u) & ~1u);
    const size_t offCount = n * sizeof(int32_t), offWeights = offCount + n * sizeof(uint32_t), bytes = offWeights + n * stride * sizeof(int16_t);
    std::vector<uint8_t> host(bytes, 0);
    memcpy(host.data(), first.data(), n * sizeof(int32_t));
    memcpy(host.data() + offCount, count.data(), n * sizeof(uint32_t));
    for (size_t p = 0; p < n; ++p)
        memcpy(host.data() + offWeights + p * stride * sizeof(int16_t), &weights[p * LFG_RESAMPLE_MAX_TAPS], count[p] * sizeof(int16_t));
    const int up = upload_table(ctx, host.data(), bytes, "resample table", &t.d_base);
    if (up != LFG_OK) return up;
    t.axis.first = reinterpret_cast<const int32_t *>(t.d_base);
    t.axis.count = reinterpret_cast<const uint32_t *>(t.d_base + offCount);
    t.axis.weights = reinterpret_cast<const int16_t *>(t.d_base + offWeights);
    t.axis.stride = stride;
    ctx->resample_tables.insert(t);
    *out = t;
    return LFG_OK;
}

// What lfg_resample, lfg_resample_antiring and lfg_upscale_edge ask of their two frames before anything else.
int resample_frames(lfg_context *ctx, const lfg_frame *in, const lfg_frame *out, const char *who) {
    if (!frame_ok(in, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, std::string(who) + ": in and out must be non-empty RGBA8");
    if ((in->pitch | out->pitch) % 4u || ((uintptr_t)in->data | (uintptr_t)out->data) % 4u)
        return fail(ctx, LFG_ERR_INVALID, std::string(who) + ": RGBA8 frames must be 4-byte aligned with a pitch that is a multiple of 4");
    return LFG_OK;
}

// The tables of one mode of lfg_resample_light on the device -- forward[256] | threshold[255], 0xFFFF as uint16_t, 1 KiB --
// built with lfg_light_tables and uploaded at the mode's first use; the context keeps both until it is destroyed.
int light_table(lfg_context *ctx, int light, const uint32_t **out) {
    uint32_t *&slot = ctx->light_tables[light - LFG_LIGHT_LINEAR];
    if (!slot) {
        uint16_t host[2 * lfg::kLightLevels];
        if (lfg_light_tables(light, host, host + lfg::kLightLevels) != LFG_OK) return fail(ctx, LFG_ERR_INVALID, "lfg_resample_light: no tables for this light");
        host[2 * lfg::kLightLevels - 1] = 0xFFFFu;
        uint8_t *d = nullptr;
        const int rc = upload_table(ctx, host, sizeof host, "light tables", &d);
        if (rc != LFG_OK) return rc;
        slot = reinterpret_cast<uint32_t *>(d);
    }
    *out = slot;
    return LFG_OK;
}

// lfg_resample (strength 0, LFG_LIGHT_GAMMA), lfg_resample_antiring and lfg_resample_light: the checks, the tables and the one
// launch.  A pass is anti-ringed where the strength is positive, the filter has weights to ring with and the pass's axis grows;
// the sums are formed in another light where one is asked for and the filter has sums to form; where neither holds, this is
// lfg_resample: the same kernel and the same launch.
int resample_call(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter, int strength, int light, const char *who) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    const int frames = resample_frames(ctx, in, out, who);
    if (frames != LFG_OK) return frames;
    if (!resample_filter_known(filter)) return fail(ctx, LFG_ERR_INVALID, std::string(who) + ": unknown filter");
    if (strength < 0 || strength > 64) return fail(ctx, LFG_ERR_INVALID, std::string(who) + ": strength must be in [0, 64]");
    if (light < LFG_LIGHT_GAMMA || light > LFG_LIGHT_SIGMOID) return fail(ctx, LFG_ERR_INVALID, std::string(who) + ": unknown light");
    if (frames_overlap(in, out)) return fail(ctx, LFG_ERR_INVALID, std::string(who) + ": the output overlaps the input");
    if (filter == LFG_FILTER_NEAREST) light = LFG_LIGHT_GAMMA;          // one tap: the tables round-trip
    if (light == LFG_LIGHT_SIGMOID && (out->width < in->width || out->height < in->height))
        return fail(ctx, LFG_ERR_UNSUPPORTED, std::string(who) + ": sigmoidal light is for upscaling; an axis that shrinks is averaged in linear light");
    trim_tables(ctx, ctx->resample_tables);
    trim_tables(ctx, ctx->resample_brackets);
    lfg::ResampleTable tx, ty;
    int rc = resample_table(ctx, filter, in->width, out->width, &tx);
    if (rc == LFG_OK) rc = resample_table(ctx, filter, in->height, out->height, &ty);
    if (rc != LFG_OK) return rc;
    const bool rings = strength > 0 && filter != LFG_FILTER_NEAREST;
    const int sx = rings && out->width > in->width ? strength : 0, sy = rings && out->height > in->height ? strength : 0;
    lfg::ResampleBracket bx{}, by{};
    if (sx) rc = resample_bracket_table(ctx, in->width, out->width, &bx);
    if (sy && rc == LFG_OK) rc = resample_bracket_table(ctx, in->height, out->height, &by);
    const uint32_t *lt = nullptr;
    if (light != LFG_LIGHT_GAMMA && rc == LFG_OK) rc = light_table(ctx, light, &lt);
    if (rc != LFG_OK) return rc;
    StageTimer timer(ctx, LFG_STAGE_SCALE);
    const hipError_t e = lt       ? lfg::launch_resample_light(ctx->cur().stream, *in, *out, tx.axis, ty.axis, ty.plan, lt)
                         : sx || sy ? lfg::launch_resample_antiring(ctx->cur().stream, *in, *out, tx.axis, ty.axis, ty.plan, bx, by, sx, sy)
                                    : lfg::launch_resample(ctx->cur().stream, *in, *out, tx.axis, ty.axis, ty.plan);
    if (e != hipSuccess) return fail_hip(ctx, e, "resample kernel launch");
    return LFG_OK;
}

}  // namespace

LFG_EXPORT int lfg_resample(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter) {
    return resample_call(ctx, in, out, filter, 0, LFG_LIGHT_GAMMA, "lfg_resample");
}

LFG_EXPORT int lfg_resample_antiring(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter, int strength) {
    return resample_call(ctx, in, out, filter, strength, LFG_LIGHT_GAMMA, "lfg_resample_antiring");
}

LFG_EXPORT int lfg_resample_light(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter, int light) {
    return resample_call(ctx, in, out, filter, 0, light, "lfg_resample_light");
}

// ---- edge-adaptive upscaling (upscale_edge.hip)

LFG_EXPORT int lfg_upscale_edge_positions(uint32_t in_size, uint32_t out_size, int32_t *base, uint8_t *frac) {
    if (!base || !frac || in_size == 0 || out_size == 0 || in_size > 0x7fffffffu || out_size > 0x7fffffffu) return LFG_ERR_INVALID;
    const int64_t in = in_size, out = out_size, D = 2 * out;
    for (uint32_t p = 0; p < out_size; ++p) {
        const int64_t N = (2 * (int64_t)p + 1) * in - out;             // below 2^63: both sizes are below 2^31
        const int64_t a = N >= 0 ? N / D : -((-N + D - 1) / D);
        base[p] = (int32_t)a;
        frac[p] = (uint8_t)((256 * (N - a * D)) / D);
    }
    return LFG_OK;
}

LFG_EXPORT int lfg_upscale_edge_shapes(int16_t *shapes) {
    if (!shapes) return LFG_ERR_INVALID;
    static const int kCos[lfg::kEdgeDirections] = {256, 251, 237, 213, 181, 142, 98, 50, 0, -50, -98, -142, -181, -213, -237, -251};
    static const int kSin[lfg::kEdgeDirections] = {0, 50, 98, 142, 181, 213, 237, 251, 256, 251, 237, 213, 181, 142, 98, 50};
    const auto floor_shift = [](int64_t v, int n) { return v >= 0 ? v >> n : -((-v + ((int64_t)1 << n) - 1) >> n); };
    for (int k = 0; k < lfg::kEdgeDirections; ++k)
        for (int q = 0; q < lfg::kEdgeStrengths; ++q) {
            const int64_t c = kCos[k], s = kSin[k], m = std::max(std::abs(kCos[k]), std::abs(kSin[k]));
            const int64_t stretch = (65536 + m / 2) / m, len = q * q;
            const int64_t sx = 256 + (((stretch - 256) * len) >> 10), sy = 256 - (len >> 3), lob = 2048 - ((1188 * len) >> 10);
            int16_t *row = shapes + (size_t)(k * lfg::kEdgeStrengths + q) * 5u;
            row[0] = (int16_t)((sx * sx * c * c + sy * sy * s * s) >> 22);
            row[1] = (int16_t)floor_shift((sx * sx - sy * sy) * c * s, 22);
            row[2] = (int16_t)((sx * sx * s * s + sy * sy * c * c) >> 22);
            row[3] = (int16_t)lob;
            row[4] = (int16_t)(((int64_t)1 << 24) / lob);
        }
    return LFG_OK;
}

namespace {

// The positions of one axis, built and uploaded at their first use.  The kernel sizes a tile's LDS on the strength of
//   0 <= base[p + 1] - base[p] <= 1   and   -1 <= base[p] <= in - 1,
// which hold because out >= in and are asserted here on what the builder returned.
int edge_position_table(lfg_context *ctx, uint32_t in_size, uint32_t out_size, lfg::EdgeAxis *out) {
    if (const auto hit = ctx->edge_positions.find(std::make_pair(in_size, out_size))) { *out = hit->axis; return LFG_OK; }
    const size_t n = out_size;
    std::vector<uint8_t> host(5 * n);                              // base | frac
    int32_t *base = reinterpret_cast<int32_t *>(host.data());
    if (lfg_upscale_edge_positions(in_size, out_size, base, host.data() + 4 * n) != LFG_OK)
        return fail(ctx, LFG_ERR_INVALID, "lfg_upscale_edge: a frame of this size has no positions");
    for (size_t p = 0; p < n; ++p)
        if (base[p] < -1 || (int64_t)base[p] > (int64_t)in_size - 1 || (p > 0 && (base[p] < base[p - 1] || base[p] > base[p - 1] + 1)))
            return fail(ctx, LFG_ERR_INVALID, "lfg_upscale_edge: positions that leave a tile's span (" + std::to_string(in_size) + " -> " +
                                                  std::to_string(out_size) + ", sample " + std::to_string(p) + ")");
    lfg::EdgePositionTable t;
    t.in_size = in_size; t.out_size = out_size;
    const int rc = upload_table(ctx, host.data(), host.size(), "edge positions", &t.d_base);
    if (rc != LFG_OK) return rc;
    t.axis.base = reinterpret_cast<const int32_t *>(t.d_base);
    t.axis.frac = t.d_base + 4 * n;
    ctx->edge_positions.insert(t);
    *out = t.axis;
    return LFG_OK;
}

// The shape table on the device, rows padded to 16 bytes: made once per context.
int edge_shape_table(lfg_context *ctx) {
    if (ctx->edge_shapes) return LFG_OK;
    constexpr size_t kRows = (size_t)lfg::kEdgeDirections * lfg::kEdgeStrengths;
    std::vector<int16_t> rows(kRows * 5u);
    std::vector<lfg::EdgeShape> host(kRows);
    if (lfg_upscale_edge_shapes(rows.data()) != LFG_OK) return fail(ctx, LFG_ERR_INVALID, "lfg_upscale_edge: no shape table");
    for (size_t i = 0; i < kRows; ++i) host[i] = lfg::EdgeShape{rows[5 * i], rows[5 * i + 1], rows[5 * i + 2], rows[5 * i + 3], rows[5 * i + 4], {0, 0, 0}};
    uint8_t *d = nullptr;
    const int rc = upload_table(ctx, host.data(), kRows * sizeof(lfg::EdgeShape), "edge shapes", &d);
    if (rc == LFG_OK) ctx->edge_shapes = reinterpret_cast<lfg::EdgeShape *>(d);
    return rc;
}

}  // namespace

LFG_EXPORT int lfg_upscale_edge(lfg_context *ctx, const lfg_frame *in, lfg_frame *out) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    int rc = resample_frames(ctx, in, out, "lfg_upscale_edge");
    if (rc != LFG_OK) return rc;
    if (frames_overlap(in, out)) return fail(ctx, LFG_ERR_INVALID, "lfg_upscale_edge: the output overlaps the input");
    if (out->width < in->width || out->height < in->height)
        return fail(ctx, LFG_ERR_UNSUPPORTED, "lfg_upscale_edge: the output is smaller than the input on an axis (lfg_resample shrinks)");
    trim_tables(ctx, ctx->edge_positions);
    lfg::EdgeAxis x{}, y{};
    rc = edge_position_table(ctx, in->width, out->width, &x);
    if (rc == LFG_OK) rc = edge_position_table(ctx, in->height, out->height, &y);
    if (rc == LFG_OK) rc = edge_shape_table(ctx);
    if (rc != LFG_OK) return rc;
    StageTimer timer(ctx, LFG_STAGE_SCALE);
    const hipError_t e = lfg::launch_upscale_edge(ctx->cur().stream, *in, *out, x, y, ctx->edge_shapes);
    if (e != hipSuccess) return fail_hip(ctx, e, "upscale_edge kernel launch");
    return LFG_OK;
}

LFG_EXPORT int lfg_set_fused_motion_interpolate(lfg_context *ctx, int enabled) {
    if (!ctx) return LFG_ERR_INVALID;
    ctx->fuse_motion_interpolate = enabled != 0;
    return LFG_OK;
}

LFG_EXPORT int lfg_set_fused_interpolate_scale(lfg_context *ctx, int enabled) {
    if (!ctx) return LFG_ERR_INVALID;
    ctx->fuse_interpolate_scale = enabled != 0;
    return LFG_OK;
}

LFG_EXPORT int lfg_interpolate_scale(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                     lfg_frame *out, float factor) {
    if (!ctx) return LFG_ERR_INVALID;
    LFG_HIP(ctx, hipSetDevice(ctx->device));
    if (!frame_ok(prev, LFG_FORMAT_RGBA8_UNORM) || !frame_ok(curr, LFG_FORMAT_RGBA8_UNORM) ||
        !frame_ok(mv, LFG_FORMAT_MV_S8X2) || !frame_ok(out, LFG_FORMAT_RGBA8_UNORM))
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_scale: bad frame (NULL, empty or wrong format)");
    if (!same_size(prev, curr) || !same_size(curr, mv))
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_scale: prev, curr and mv differ in size");
    if ((prev->pitch | curr->pitch) % 4u || mv->pitch % 2u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_scale: row pitch not a multiple of the pixel size");
    if (out->data == prev->data || out->data == curr->data)
        return fail(ctx, LFG_ERR_INVALID, "lfg_interpolate_scale: output aliases an input");
    trim_tables(ctx, ctx->tables);
    lfg::AxisTable tx, ty;
    int rc = build_axis_table(ctx, (int)curr->width, (int)out->width, &tx);
    if (rc != LFG_OK) return rc;
    rc = build_axis_table(ctx, (int)curr->height, (int)out->height, &ty);
    if (rc != LFG_OK) return rc;
    const bool fused = ctx->fuse_interpolate_scale && tx.pattern_2x && ty.pattern_2x && tx.palette_rows > 0 && ty.strips_per_xcd > 0 && lfg::scale_2x_supported(*curr, *out) &&
                       (uint64_t)prev->height * prev->pitch < 0x7fffffffull;
    if (fused) {
        // one kernel: the generated frame is interpolated row by row inside the 2x scale kernel and never stored at
        // input resolution; accounted to the scale stage
        StageTimer timer(ctx, LFG_STAGE_SCALE);
        hipError_t e = lfg::launch_interpolate_scale_2x(ctx->cur().stream, *prev, *curr, *mv, *out, tx, ty, factor, ctx->semantics != 0);
        if (e != hipSuccess) return fail_hip(ctx, e, "fused interpolate + scale kernel launch");
        ctx->scale_last_kernel = 2;
        return LFG_OK;
    }
    // any other size ratio: the two stages, through a context-owned frame at input resolution
    lfg_frame &mid = ctx->cur().mid_tmp;
    rc = lane_frame(ctx, mid, curr->width, curr->height, LFG_FORMAT_RGBA8_UNORM);
    if (rc != LFG_OK) return rc;
    rc = lfg_interpolate(ctx, prev, curr, mv, &mid, factor);
    if (rc != LFG_OK) return rc;
    return lfg_scale(ctx, &mid, out);
}

LFG_EXPORT int lfg_mv_export_rgba32f(lfg_context *ctx, const lfg_frame *mv, void *device_rgba32f) {
    if (!ctx || !frame_ok(mv, LFG_FORMAT_MV_S8X2) || !device_rgba32f || (uintptr_t)device_rgba32f % 16u)
        return fail(ctx, LFG_ERR_INVALID, "lfg_mv_export_rgba32f: bad argument");
    hipError_t e = lfg::launch_mv_export(ctx->cur().stream, *mv, (float *)device_rgba32f);
    if (e != hipSuccess) return fail_hip(ctx, e, "mv export kernel launch");
    return LFG_OK;
}

// ================================================================== diagnostics

LFG_EXPORT int lfg_selftest_sqrt(lfg_context *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t *out_mismatches) {
    if (!ctx || !out_mismatches || lo_bits > hi_bits) return fail(ctx, LFG_ERR_INVALID, "lfg_selftest_sqrt: bad argument");
    unsigned long long *d = nullptr;
    LFG_HIP(ctx, hipMalloc((void **)&d, sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->cur().stream);
    if (e == hipSuccess) e = lfg::launch_sqrt_selftest(ctx->cur().stream, lo_bits, hi_bits, d);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, ctx->cur().stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->cur().stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail_hip(ctx, e, "sqrt selftest");
    *out_mismatches = (uint64_t)h;
    return LFG_OK;
}

LFG_EXPORT int lfg_diag_scale_2x_strip(uint32_t in_height, uint32_t xcd, uint32_t index, uint32_t *out_strips_per_xcd,
                                       int32_t *out_first_step, int32_t *out_steps) {
    if (in_height == 0 || in_height > 32768u || xcd >= 8u) return LFG_ERR_INVALID;
    const int per = lfg::scale_2x_strips_per_xcd((int)in_height);
    if (out_strips_per_xcd) *out_strips_per_xcd = (uint32_t)per;
    if ((int)index >= per) return LFG_ERR_INVALID;
    int first = 0, steps = 0;
    lfg::scale_2x_strip_host((int)in_height, (int)xcd, (int)index, first, steps);
    if (out_first_step) *out_first_step = first;
    if (out_steps) *out_steps = steps;
    return LFG_OK;
}

// ================================================================== measurement

LFG_EXPORT int lfg_profile_enable(lfg_context *ctx, int enabled) {
    if (!ctx) return LFG_ERR_INVALID;
    int rc = drain_profile(ctx);
    ctx->profile = enabled != 0;
    return rc;
}

LFG_EXPORT int lfg_profile_reset(lfg_context *ctx) {
    if (!ctx) return LFG_ERR_INVALID;
    int rc = drain_profile(ctx);
    for (int i = 0; i < LFG_STAGE_COUNT; ++i) { ctx->prof_ms[i] = 0.0; ctx->prof_n[i] = 0; }
    return rc;
}

LFG_EXPORT int lfg_profile_get(lfg_context *ctx, int stage, double *out_total_ms, uint64_t *out_launches) {
    if (!ctx || stage < 0 || stage >= LFG_STAGE_COUNT) return LFG_ERR_INVALID;
    int rc = drain_profile(ctx);
    if (out_total_ms) *out_total_ms = ctx->prof_ms[stage];
    if (out_launches) *out_launches = ctx->prof_n[stage];
    return rc;
}
