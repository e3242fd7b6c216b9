#include "evaluate.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>

namespace {

lfg_context* Ctx() { return HipContext::Get().GetDevice(); }

constexpr uint32_t kMask = 0xF;

std::string SummaryJson(const lfg_frame_diff_stats& s, const lfg_frame_diff_summary& m) {
    char psnr[64], text[640];
    if (std::isinf(m.psnr_db)) snprintf(psnr, sizeof psnr, "null");
    else snprintf(psnr, sizeof psnr, "%.17g", m.psnr_db);
    snprintf(text, sizeof text,
             "{\"pixels\": %llu, \"differing\": %llu, \"over_1\": %llu, \"max_abs\": %u, \"p50\": %u, \"p99\": %u, \"mse\": %.17g, "
             "\"psnr_db\": %s, \"sse\": [%llu, %llu, %llu, %llu]}",
             (unsigned long long)m.pixels, (unsigned long long)m.differing, (unsigned long long)m.over_1, m.max_abs, m.p50, m.p99,
             m.mse, psnr, (unsigned long long)s.sse[0], (unsigned long long)s.sse[1], (unsigned long long)s.sse[2],
             (unsigned long long)s.sse[3]);
    return text;
}

// The "ssim" value of a summary object: the record's figures, or null where the output is too small for a window.
std::string SsimJson(bool measured, const lfg_frame_ssim_stats& s, const lfg_frame_ssim_summary& m) {
    if (!measured) return "null";
    char db[64], text[960];
    if (std::isinf(m.db)) snprintf(db, sizeof db, "null");
    else snprintf(db, sizeof db, "%.17g", m.db);
    snprintf(text, sizeof text,
             "{\"windows\": %llu, \"all\": %.17g, \"db\": %s, \"channels\": [%.17g, %.17g, %.17g, %.17g], "
             "\"sum\": [%lld, %lld, %lld, %lld], \"identical\": %llu, \"below_half\": %llu, "
             "\"worst\": {\"value\": %.17g, \"x\": %u, \"y\": %u}}",
             (unsigned long long)m.windows, m.all, db, m.ssim[0], m.ssim[1], m.ssim[2], m.ssim[3], (long long)s.sum[0],
             (long long)s.sum[1], (long long)s.sum[2], (long long)s.sum[3], (unsigned long long)m.identical,
             (unsigned long long)m.below_half, m.worst_value, m.worst_x, m.worst_y);
    return text;
}

// A summary object with "ssim" behind its last key.
std::string WithSsim(std::string summary, const std::string& ssim) {
    summary.insert(summary.size() - 1, ", \"ssim\": " + ssim);
    return summary;
}

// Everything the loop owns, released on every way out.
struct Resources {
    Frame input, up[3], out, records;
    lfg_ring* ring = nullptr;
    void* host = nullptr;
    ~Resources() {
        auto& fm = FrameManager::Get();
        if (ring) lfg_ring_destroy(ring);
        if (host) fm.DestroyStagingBuffer(host);
        for (Frame* f : {&input, &up[0], &up[1], &up[2], &out, &records}) fm.DestroyFrame(*f);
    }
};

}  // namespace

bool RunEvaluation(FrameSource& source, uint32_t inputWidth, uint32_t inputHeight, uint32_t outputWidth, uint32_t outputHeight,
                   int frames, EvaluationResult& result, bool extrapolate, int scaleFilter) {
    auto& fm = FrameManager::Get();
    if (!Ctx() || frames < 3) {
        LOG_ERROR("RunEvaluation: needs an initialized HipContext and at least 3 frames");
        return false;
    }
    if (!source.Initialize(inputWidth, inputHeight)) {
        LOG_ERROR("Failed to initialize frame source");
        return false;
    }
    Resources r;
    const size_t inBytes = (size_t)inputWidth * inputHeight * 4, diffBytes = 2 * sizeof(lfg_frame_diff_stats);
    const size_t recordBytes = diffBytes + 2 * sizeof(lfg_frame_ssim_stats);
    const bool ssim = outputWidth >= 8 && outputHeight >= 8;    // lfg_frame_ssim's smallest frame: one window
    bool ok = fm.CreateFrame(r.input, inputWidth, inputHeight) && fm.CreateFrame(r.out, outputWidth, outputHeight) &&
              fm.CreateFrame(r.records, (uint32_t)(recordBytes / 4), 1) && fm.CreateStagingBuffer(r.host, recordBytes);
    for (Frame& f : r.up) ok = ok && fm.CreateFrame(f, outputWidth, outputHeight);
    if (!ok || lfg_lanes(Ctx(), 1) != LFG_OK || lfg_ring_create(Ctx(), 3, inBytes, &r.ring) != LFG_OK) {
        LOG_ERROR("Failed to create the evaluation's frames: ", lfg_last_error(Ctx()));
        return false;
    }
    void* generated = r.records.data;
    void* repeated = static_cast<uint8_t*>(r.records.data) + sizeof(lfg_frame_diff_stats);
    void* generatedSsim = static_cast<uint8_t*>(r.records.data) + diffBytes;
    void* repeatedSsim = static_cast<uint8_t*>(generatedSsim) + sizeof(lfg_frame_ssim_stats);
    // lfg_frame_ssim beside a lfg_frame_diff, into the record of its own
    auto similar = [&](const lfg_frame& x, const lfg_frame& y, uint64_t k, void* record) {
        return !ssim || lfg_frame_ssim(Ctx(), &x, &y, kMask, k > 0 ? 1 : 0, record) == LFG_OK;
    };

    // the next source frame, upscaled into `into`: the upload is ordered behind the scale that last read r.input
    auto next = [&](Frame& into) {
        void* slotHost = nullptr;
        uint32_t slot = 0;
        if (lfg_ring_acquire(r.ring, &slotHost, &slot) != LFG_OK) { LOG_ERROR("Failed to acquire an upload slot"); return false; }
        if (!source.NextFrame(static_cast<uint8_t*>(slotHost))) { LOG_ERROR("Failed to capture frame"); return false; }
        lfg_frame in = r.input.AsAbi(), up = into.AsAbi();
        if (lfg_ring_upload(r.ring, slot, &in) != LFG_OK ||
            (scaleFilter < 0 ? lfg_scale(Ctx(), &in, &up) : lfg_resample(Ctx(), &in, &up, scaleFilter)) != LFG_OK) {
            LOG_ERROR("Failed to upload and upscale a frame: ", lfg_last_error(Ctx()));
            return false;
        }
        return true;
    };

    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t pairs = (uint64_t)(frames - 1) / 2;
    Frame *prev = &r.up[0], *held = &r.up[1], *curr = &r.up[2];
    if (!next(*prev)) return false;
    for (uint64_t k = 0; k < pairs; ++k) {
        if (!next(*held) || !next(*curr)) return false;
        const lfg_frame p = prev->AsAbi(), h = held->AsAbi(), c = curr->AsAbi();
        lfg_frame o = r.out.AsAbi();
        // interpolate: frames 2k and 2k + 2 give 2k + 1.  extrapolate: frames 2k and 2k + 1 give 2k + 2, one interval ahead of
        // the newest frame, and the yardstick is that newest frame shown again
        const bool enqueued = extrapolate ? lfg_interpolate_frames(Ctx(), &p, &h, &o, 1.0f) == LFG_OK &&
                                                lfg_frame_diff(Ctx(), &o, &c, kMask, k > 0 ? 1 : 0, generated) == LFG_OK && similar(o, c, k, generatedSsim) &&
                                                lfg_frame_diff(Ctx(), &h, &c, kMask, k > 0 ? 1 : 0, repeated) == LFG_OK && similar(h, c, k, repeatedSsim)
                                          : lfg_interpolate_frames(Ctx(), &p, &c, &o, 0.5f) == LFG_OK &&
                                                lfg_frame_diff(Ctx(), &o, &h, kMask, k > 0 ? 1 : 0, generated) == LFG_OK && similar(o, h, k, generatedSsim) &&
                                                lfg_frame_diff(Ctx(), &p, &h, kMask, k > 0 ? 1 : 0, repeated) == LFG_OK && similar(p, h, k, repeatedSsim);
        if (!enqueued) {
            LOG_ERROR("Failed to enqueue pair ", k, ": ", lfg_last_error(Ctx()));
            return false;
        }
        std::swap(prev, curr);                               // frame 2k + 2 is the next pair's first
    }
    const lfg_frame rec = r.records.AsAbi();
    if (lfg_frame_download(Ctx(), &rec, r.host, recordBytes) != LFG_OK || lfg_sync(Ctx()) != LFG_OK) {
        LOG_ERROR("Failed to read the records back: ", lfg_last_error(Ctx()));
        return false;
    }
    result.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    lfg_frame_diff_stats stats[2];
    lfg_frame_diff_summary summary[2];
    lfg_frame_ssim_stats ssimStats[2];
    lfg_frame_ssim_summary ssimSummary[2] = {};
    memcpy(stats, r.host, diffBytes);
    memcpy(ssimStats, static_cast<uint8_t*>(r.host) + diffBytes, sizeof ssimStats);
    for (int i = 0; i < 2; ++i)
        if (lfg_frame_diff_summarize(&stats[i], kMask, &summary[i]) != LFG_OK ||
            (ssim && lfg_frame_ssim_summarize(&ssimStats[i], kMask, &ssimSummary[i]) != LFG_OK)) {
            LOG_ERROR("The ", i == 0 ? "generated" : "repeated", " record is inconsistent");
            return false;
        }
    result.pairs = pairs;
    result.json = "{\"pairs\": " + std::to_string(pairs) + ", \"generated\": " +
                  WithSsim(SummaryJson(stats[0], summary[0]), SsimJson(ssim, ssimStats[0], ssimSummary[0])) + ", \"repeated\": " +
                  WithSsim(SummaryJson(stats[1], summary[1]), SsimJson(ssim, ssimStats[1], ssimSummary[1])) + "}";
    return true;
}
