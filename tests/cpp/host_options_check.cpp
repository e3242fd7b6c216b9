// host/options.cpp compiled with g++ alone (it calls nothing in the library):
//   host_options_check parse ARGS...   every field of the Options that ARGS parse to, as one JSON line; or "refused: MESSAGE"
//   host_options_check check ARGS...   what CheckOptions says of them ("" if nothing), with a tap limit that every ratio up to 8 : 1 meets
//   host_options_check report          ReportLine against the report's former form, lfg_host's two printf statements, byte for byte
//   host_options_check usage           the option table against the usage text
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "options.hpp"

static const char* const kScaleFilterNames[6] = {"nearest", "bilinear", "catmull-rom", "mitchell", "lanczos2", "lanczos3"};

// The report as main wrote it before ReportLine: both statements verbatim, with the variables they read.
static std::string FormerReport(const Options& o, const ReportCounters& c) {
    const ScalerConfig& config = o.config;
    const int frames = o.frames, replay = o.replay, inFlight = o.inFlight, staticTolerance = o.route.staticTolerance;
    const int bidirectional = o.route.bidirectional, halfResMotion = o.route.halfResMotion, holeReach = o.route.holeReach, subpelVectors = o.route.subpelVectors;
    const bool presentNull = o.presentNull, syncPresent = o.syncPresent, inputNv12 = o.inputNv12, outputNv12 = o.outputNv12;
    char* text = nullptr;
    size_t size = 0;
    FILE* report = open_memstream(&text, &size);
    if (o.evaluate) {
        struct { uint64_t pairs; double seconds; std::string json; } result = {c.generated, c.seconds, c.evaluation};
        char filterField[136] = "";
        int used = 0;
        if (config.scaleFilter >= 0) used = snprintf(filterField, sizeof filterField, "\"scale_filter\": \"%s\", ", kScaleFilterNames[config.scaleFilter]);
        if (bidirectional >= 0) used += snprintf(filterField + used, sizeof filterField - (size_t)used, "\"bidirectional\": %d, ", bidirectional);
        if (halfResMotion >= 0) used += snprintf(filterField + used, sizeof filterField - (size_t)used, "\"half_res_motion\": %d, ", halfResMotion);
        if (holeReach >= 1) used += snprintf(filterField + used, sizeof filterField - (size_t)used, "\"hole_reach\": %d, ", holeReach);
        if (subpelVectors >= 0) snprintf(filterField + used, sizeof filterField - (size_t)used, "\"subpel_vectors\": %d, ", subpelVectors);
        fprintf(report, "{\"input_frames\": %d, \"presented\": 0, \"interpolated\": %llu, \"cuts\": 0, \"seconds\": %.4f, "
               "\"presented_fps\": 0.00, \"checksum\": 0, \"pipelined\": false, \"replay\": 0, \"present_null\": %s, \"in_flight\": 1, "
               "\"input_format\": \"rgba\", \"output_format\": \"rgba\", \"protect_static\": %d, %s"
               "\"note\": \"nothing is presented: every second source frame is held out and compared on the GPU\", \"evaluation\": %s}\n",
               frames, (unsigned long long)result.pairs, result.seconds, presentNull ? "true" : "false", staticTolerance, filterField, result.json.c_str());
    } else {
        const uint64_t presented = c.presented, generated = c.generated, cuts = c.cuts, checksum = c.checksum;
        const double sec = c.seconds;
        char sharpenField[32] = "";
        if (config.sharpen > 0) snprintf(sharpenField, sizeof sharpenField, "\"sharpen\": %u, ", config.sharpen);
        char filterField[48] = "";
        if (config.scaleFilter >= 0) snprintf(filterField, sizeof filterField, "\"scale_filter\": \"%s\", ", kScaleFilterNames[config.scaleFilter]);
        char routeFields[120] = "";
        int used = 0;
        if (bidirectional >= 0) used = snprintf(routeFields, sizeof routeFields, "\"bidirectional\": %d, ", bidirectional);
        if (halfResMotion >= 0) used += snprintf(routeFields + used, sizeof routeFields - (size_t)used, "\"half_res_motion\": %d, ", halfResMotion);
        if (holeReach >= 1) used += snprintf(routeFields + used, sizeof routeFields - (size_t)used, "\"hole_reach\": %d, ", holeReach);
        if (subpelVectors >= 0) snprintf(routeFields + used, sizeof routeFields - (size_t)used, "\"subpel_vectors\": %d, ", subpelVectors);
        fprintf(report, "{\"input_frames\": %d, \"presented\": %llu, \"interpolated\": %llu, \"cuts\": %llu, \"seconds\": %.4f, "
               "\"presented_fps\": %.2f, \"checksum\": %llu, \"pipelined\": %s, \"replay\": %d, \"present_null\": %s, \"in_flight\": %d, "
               "\"input_format\": \"%s\", \"output_format\": \"%s\", \"protect_static\": %d, %s%s%s"
               "\"note\": \"includes %s, PCIe upload and readback\"}\n",
               frames, (unsigned long long)presented, (unsigned long long)generated, (unsigned long long)cuts, sec, presented / sec,
               (unsigned long long)checksum, syncPresent ? "false" : "true", replay, presentNull ? "true" : "false", inFlight,
               inputNv12 ? "nv12" : "rgba", outputNv12 ? "nv12" : "rgba", staticTolerance, sharpenField, filterField, routeFields,
               replay > 0 ? "one memcpy per input frame into the staging slot" : "host frame synthesis");
    }
    fclose(report);
    const std::string line(text, size);
    free(text);
    return line;
}

// Every subset of the six optional fields, each present one at its least and at its greatest value; both branches; both formats at
// both doors; replay 0 and 8; small and large 64-bit counters; the flags the line shows.
static int CheckReport() {
    const int off = -1, sharpen[3] = {0, 1, 64}, filter[3] = {off, LFG_FILTER_CATMULL_ROM, LFG_FILTER_LANCZOS3}, bidirectional[3] = {off, 0, 64};
    const int halfRes[3] = {off, 0, 2}, reach[3] = {off, 1, LFG_HOLE_REACH_MAX}, subpel[3] = {off, 0, 2};
    long lines = 0;
    for (int fields = 0; fields < 729; ++fields)
        for (int flags = 0; flags < 128; ++flags) {
            Options o;
            o.config.sharpen = (uint32_t)sharpen[fields % 3];
            o.config.scaleFilter = filter[fields / 3 % 3];
            o.route.bidirectional = bidirectional[fields / 9 % 3];
            o.route.halfResMotion = halfRes[fields / 27 % 3];
            o.route.holeReach = reach[fields / 81 % 3];
            o.route.subpelVectors = subpel[fields / 243 % 3];
            o.evaluate = flags & 1;
            o.inputNv12 = flags & 2;
            o.outputNv12 = flags & 4;
            o.replay = flags & 8 ? 8 : 0;
            o.syncPresent = flags & 16;
            o.presentNull = flags & 32;
            const bool large = flags & 64;
            o.route.staticTolerance = large ? 1020 : -1;
            o.frames = large ? 2147483647 : 3;
            o.inFlight = large ? 3 : 1;
            ReportCounters c;
            c.presented = large ? 0xFFFFFFFFFFFFFFFFull : 5;
            c.generated = large ? 0xFFFFFFFFFFFFFFFEull : 2;
            c.cuts = large ? 0x8000000000000000ull : 0;
            c.checksum = large ? 0xFEDCBA9876543210ull : 1;
            c.seconds = large ? 123456.78901 : 0.00004;
            c.evaluation = large ? "{\"pairs\": 18446744073709551614, \"generated\": {}, \"repeated\": {}}" : "{}";
            const std::string now = ReportLine(o, c), former = FormerReport(o, c);
            if (now != former) {
                printf("fields %d flags %d\n now    %s former %s", fields, flags, now.c_str(), former.c_str());
                return 1;
            }
            ++lines;
        }
    printf("ok %ld\n", lines);
    return 0;
}

// Every option of the table heads a line of the usage text or stands on such a line (--ranks, --rank and --comm-file share one),
// and every --name the usage text speaks of, anywhere, is an option of the table.
static int CheckUsage() {
    const std::string usage = kUsage;
    long found = 0;
    for (size_t r = 0; r < kOptionRowCount; ++r) {
        bool listed = false;
        for (size_t at = usage.find("\n  --"); at != std::string::npos && !listed; at = usage.find("\n  --", at + 1)) {
            const std::string line = usage.substr(at + 1, usage.find('\n', at + 1) - at - 1) + " ";
            listed = line.find(std::string(" ") + kOptionRows[r].name + " ") != std::string::npos;
        }
        if (!listed) { printf("the usage text does not list %s\n", kOptionRows[r].name); return 1; }
    }
    for (size_t at = usage.find("--"); at != std::string::npos; at = usage.find("--", at)) {
        const size_t end = usage.find_first_not_of("abcdefghijklmnopqrstuvwxyz0123456789-", at);
        const std::string name = usage.substr(at, end - at);
        at = end;
        if (name == "--") continue;                    // a dash in the prose
        bool known = false;
        for (size_t r = 0; r < kOptionRowCount; ++r) known = known || name == kOptionRows[r].name;
        if (!known) { printf("the usage text names %s, which is no option\n", name.c_str()); return 1; }
        ++found;
    }
    printf("ok %zu %ld\n", kOptionRowCount, found);
    return 0;
}

static void PrintOptions(const Options& o) {
    const auto text = [](const std::string& s) { return "\"" + s + "\""; };
    std::string factors;
    char number[32];
    for (float f : o.factors) { snprintf(number, sizeof number, "%s%.9g", factors.empty() ? "" : ", ", f); factors += number; }
    printf("{\"inputWidth\": %u, \"inputHeight\": %u, \"outputWidth\": %u, \"outputHeight\": %u, \"targetFps\": %u, \"enableInterpolation\": %d, "
           "\"interpolationFactor\": %.9g, \"sharpen\": %u, \"scaleFilter\": %d, ",
           o.config.inputWidth, o.config.inputHeight, o.config.outputWidth, o.config.outputHeight, o.config.targetFps, o.config.enableInterpolation,
           o.config.interpolationFactor, o.config.sharpen, o.config.scaleFilter);
    printf("\"estimator\": %d, \"semantics\": %d, \"interpolator\": %d, \"generation\": %d, \"refineRadius\": %d, \"cutThreshold\": %d, "
           "\"staticTolerance\": %d, \"bidirectional\": %d, \"halfResMotion\": %d, \"holeReach\": %d, \"subpelVectors\": %d, ",
           o.route.estimator, o.route.semantics, o.route.interpolator, o.route.generation, o.route.refineRadius, o.route.cutThreshold,
           o.route.staticTolerance, o.route.bidirectional, o.route.halfResMotion, o.route.holeReach, o.route.subpelVectors);
    printf("\"inputNv12\": %d, \"outputNv12\": %d, \"yuvMatrix\": %d, \"yuvRange\": %d, \"yuvSiting\": %d, \"factors\": [%s], \"inFlight\": %d, "
           "\"ranks\": %d, \"rank\": %d, \"commFile\": %s, \"commNonce\": %llu, \"frames\": %d, \"device\": %d, \"replay\": %d, \"stream\": %u, ",
           o.inputNv12, o.outputNv12, o.yuv.matrix, o.yuv.range, o.yuv.siting, factors.c_str(), o.inFlight, o.ranks, o.rank, text(o.commFile).c_str(),
           o.commNonce, o.frames, o.device, o.replay, o.stream);
    printf("\"dumpDir\": %s, \"inputRaw\": %s, \"outputRaw\": %s, \"help\": %d, \"quiet\": %d, \"evaluate\": %d, \"syncPresent\": %d, \"presentNull\": %d}\n",
           text(o.dumpDir).c_str(), text(o.inputRaw).c_str(), text(o.outputRaw).c_str(), o.help, o.quiet, o.evaluate, o.syncPresent, o.presentNull);
}

int main(int argc, char* argv[]) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "report") return CheckReport();
    if (mode == "usage") return CheckUsage();
    if (mode != "parse" && mode != "check") { printf("usage: host_options_check parse|check ARGS... | report | usage\n"); return 2; }
    Options o;
    const std::string refusal = ParseOptions(argc - 1, argv + 1, o);      // (argv[1] stands where the program's name does)
    if (!refusal.empty()) { printf("refused: %s\n", refusal.c_str()); return 1; }
    if (mode == "parse") PrintOptions(o);
    else printf("%s\n", CheckOptions(o, [](int, uint32_t in, uint32_t out) { return in <= 8 * out; }).c_str());
    return 0;
}
