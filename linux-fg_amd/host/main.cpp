// lfg_host -- headless counterpart of the reference's CLI (src/main.cpp:21-144): same option names
// and the same derivation of the output size; the X11 window id is replaced by a synthetic stream
// index and the paced SDL loop by a fixed number of frames run flat out.  What the command line says is options.cpp's;
// here: parse, check, open the device, apply the route, then measure (--evaluate) or present.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "evaluate.hpp"
#include "options.hpp"

int main(int argc, char* argv[]) {
    // (HIP's default of four hardware queues is one short of three lanes + a copy stream + a communication stream: streams that
    //  share a queue run in turn.  Before the first HIP call; an explicit setting wins.  INTEGRATION.md, "Hardware queues".)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    Options o;
    std::string refusal = ParseOptions(argc, argv, o);
    if (!refusal.empty()) { LOG_ERROR(refusal); return 1; }
    if (o.help) { std::cout << kUsage; return 0; }
    if (o.quiet) Logger::Get().SetMinLevel(Logger::Level::WARNING);
    const ScalerConfig& config = o.config;
    // Before a context is made; the tap tables are a host function of the library.
    refusal = CheckOptions(o, [](int filter, uint32_t in, uint32_t out) {
        std::vector<int32_t> first(out);
        std::vector<uint32_t> count(out);
        std::vector<int16_t> weights((size_t)out * LFG_RESAMPLE_MAX_TAPS);
        return lfg_resample_taps(filter, in, out, first.data(), count.data(), weights.data()) == LFG_OK;
    });
    if (!refusal.empty()) { LOG_ERROR(refusal); return 2; }

    if (!HipContext::Get().Initialize(o.device)) { LOG_ERROR("Failed to initialize HIP"); return 1; }
    if (!HipContext::Get().SetRoute(o.route)) { HipContext::Get().Cleanup(); return 1; }
    if (!FrameManager::Get().Initialize(config.outputWidth, config.outputHeight)) {
        LOG_ERROR("Failed to initialize frame manager");
        HipContext::Get().Cleanup();
        return 1;
    }
    const bool extrapolate = o.route.generation == LFG_GENERATION_EXTRAPOLATE;
    ReportCounters counters;
    if (o.evaluate) {
        std::unique_ptr<FrameSource> source;
        if (!o.inputRaw.empty()) source = std::make_unique<RawFileCapture>(o.inputRaw);
        else source = std::make_unique<SyntheticCapture>(o.stream);
        EvaluationResult result;
        const bool ok = RunEvaluation(*source, config.inputWidth, config.inputHeight, config.outputWidth, config.outputHeight, o.frames, result,
                                      extrapolate, config.scaleFilter);
        source.reset();
        FrameManager::Get().Cleanup();
        HipContext::Get().Cleanup();
        if (!ok) { LOG_ERROR("Evaluation failed: ", Logger::Get().GetLastError()); return 1; }
        counters.generated = result.pairs;
        counters.seconds = result.seconds;
        counters.evaluation = result.json;
        fputs(ReportLine(o, counters).c_str(), stdout);
        return 0;
    }
    if (o.ranks > 0) {
        if (o.commFile.empty() || o.rank < 0 || o.rank >= o.ranks) { LOG_ERROR("--ranks needs --rank in range and --comm-file"); return 1; }
        if (!HipContext::Get().InitComm(o.ranks, o.rank, o.commFile, (uint64_t)o.commNonce)) { HipContext::Get().Cleanup(); return 1; }
        Scaler::Get().SetSharedPreviousSource(std::make_unique<SyntheticCapture>(0));   // the batch's previous frames: stream 0
        if (o.stream == 0) o.stream = (uint32_t)o.rank + 1;                             // a rank's own current frames
    }
    {
        std::unique_ptr<FrameSource> source;
        if (!o.inputRaw.empty()) source = std::make_unique<RawFileCapture>(o.inputRaw, o.inputNv12);
        else source = std::make_unique<SyntheticCapture>(o.stream);
        if (o.replay > 0) source = std::make_unique<ReplayCapture>(std::move(source), (uint32_t)o.replay);
        Scaler::Get().SetFrameSource(std::move(source));
    }
    Scaler::Get().SetPipelined(!o.syncPresent);
    Scaler::Get().SetFramesInFlight(o.inFlight);
    Scaler::Get().SetCutCounting(o.route.cutThreshold >= 0);
    Scaler::Get().SetRealFrameFirst(extrapolate);
    Scaler::Get().SetNv12(o.inputNv12, o.outputNv12, o.yuv);
    if (!o.factors.empty()) Scaler::Get().SetInterpolationFactors(o.factors);
    FILE* rawOut = nullptr;
    if (!o.outputRaw.empty()) {
        rawOut = o.outputRaw == "-" ? stdout : fopen(o.outputRaw.c_str(), "wb");
        if (!rawOut) { LOG_ERROR("Cannot open ", o.outputRaw); return 1; }
    }
    FILE* report = rawOut == stdout ? stderr : stdout;          // keep the pixel stream clean
    Scaler::Get().SetPresenter([&](const uint8_t* rgba, uint32_t w, uint32_t h, bool interpolated) {
        const size_t n = Scaler::Get().PresentedBytes(w, h);    // (NV12 with --output-format nv12)
        uint64_t s = 0;
        if (!o.presentNull) for (size_t i = 0; i < n; i += 64) s += rgba[i];
        counters.checksum = counters.checksum * 1315423911ull + s;
        if (!o.dumpDir.empty()) {
            char name[512];
            snprintf(name, sizeof name, "%s/frame_%04llu_%s_%ux%u.%s", o.dumpDir.c_str(), (unsigned long long)counters.presented,
                     interpolated ? "interp" : "real", w, h, o.outputNv12 ? "nv12" : "rgba");
            if (FILE* f = fopen(name, "wb")) { fwrite(rgba, 1, n, f); fclose(f); }
        }
        if (rawOut) fwrite(rgba, 1, n, rawOut);
        ++counters.presented;
        counters.generated += interpolated ? 1 : 0;
    });
    if (!Scaler::Get().Initialize(config)) {
        LOG_ERROR("Failed to initialize scaler");
        FrameManager::Get().Cleanup();
        HipContext::Get().Cleanup();
        return 1;
    }

    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    for (int i = 0; i < o.frames && ok; ++i) ok = Scaler::Get().ProcessFrame();
    ok = ok && Scaler::Get().Flush();                           // the last call's frames
    counters.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    counters.cuts = Scaler::Get().GetCuts();
    // Teardown order as src/main.cpp:138-141.
    Scaler::Get().Cleanup();
    FrameManager::Get().Cleanup();
    HipContext::Get().Cleanup();
    if (!ok) { LOG_ERROR("ProcessFrame failed: ", Logger::Get().GetLastError()); return 1; }
    if (rawOut && rawOut != stdout) fclose(rawOut);
    fputs(ReportLine(o, counters).c_str(), report);
    return 0;
}
