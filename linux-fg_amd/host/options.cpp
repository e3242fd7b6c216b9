#include "options.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

const char kUsage[] =
    "Usage: lfg_host [options] [stream-index]\n"
    "Options:\n"
    "  --help                   Show this help message\n"
    "  --input-width WIDTH      Input width (default: 1920)\n"
    "  --input-height HEIGHT    Input height (default: 1080)\n"
    "  --output-width WIDTH     Output width\n"
    "  --output-height HEIGHT   Output height\n"
    "  --target-fps FPS         Accepted for compatibility; frames are not paced\n"
    "  --no-interpolation       Disable frame interpolation\n"
    "  --interpolation-factor F Interpolation blend factor (0.0-1.0, default: 0.5)\n"
    "  --factors A,B,...        Several generated frames per pair, in presentation order (e.g. 0.25,0.5,0.75\n"
    "                           for 60 -> 240 fps); motion runs once per pair\n"
    "  --in-flight N            Frames in flight on the GPU, 1..3 (default 2): a frame's upscale and first motion units\n"
    "                           run while the previous frame's last long units finish; same frames, same order\n"
    "  --ranks N --rank R --comm-file FILE\n"
    "                           One process per GPU (BASELINE config 4): the batch shares its previous frame\n"
    "                           (synthetic stream 0, captured on rank 0, broadcast over RCCL per frame); each\n"
    "                           rank's current frames are its own stream.  FILE carries the communicator id.\n"
    "  --comm-nonce N           A number the launcher gives every rank of ONE run (default: LFG_COMM_NONCE, else 0; more than one rank needs a non-zero one): an\n"
    "                           id file left behind by another run is then never joined\n"
    "  --motion full|pyramid    Motion estimator of the generated frames (default full: the reference's +-16 search;\n"
    "                           pyramid: coarse-to-fine, +-70 px at a cost independent of the content)\n"
    "  --semantics reference|intended  Arithmetic of motion and interpolation (default reference: the shaders as\n"
    "                           written; intended: vectors displace by pixels -- what vectors longer than 1 px need)\n"
    "  --interpolator shader|compensated  Interpolation of the generated frames (default shader: the reference's;\n"
    "                           compensated: vectors projected to the frame's time, holes filled; wants --semantics intended)\n"
    "  --generation interpolate|extrapolate  Where the generated frames lie (default interpolate: between the last two real\n"
    "                           frames, the newest one held back until they are shown; extrapolate: AHEAD of the newest real\n"
    "                           frame, which is presented as it arrives, each factor read as the fraction of an interval\n"
    "                           ahead).  extrapolate needs --interpolator compensated and is not available with --ranks\n"
    "  --refine-vectors R       Per-pixel vector refinement between motion and interpolation (default -1: off;\n"
    "                           0..2: each pixel takes the nearby vector that fits its (2R+1)^2 window best)\n"
    "  --cut-threshold P        Scene-cut detection (default -1: off; 0..1000: a pair of which fewer than P pixels per\n"
    "                           thousand match under its vectors shows a source frame instead of a generated one)\n"
    "  --protect-static T       Static-overlay protection of the compensated interpolator (default -1: off; 0..1020: pixels\n"
    "                           whose four channels differ by at most T in sum between the pair's frames stay where they\n"
    "                           are -- a HUD, a crosshair, text; no effect with --interpolator shader)\n"
    "  --bidirectional T        Bidirectional compensated interpolation (default -1: off; 0..64: the pair is measured both ways,\n"
    "                           a vector projects only where the two fields agree within T in L1, and both frames' grids\n"
    "                           project; doubles the motion stage.  No effect with --interpolator shader, --generation\n"
    "                           extrapolate or --protect-static)\n"
    "  --half-res-motion R      Half-resolution motion (default -1: off; 0..2: the estimator runs on both frames halved and\n"
    "                           each pixel takes the doubled vector of the 3 x 3 coarse neighbours that fits its (2R+1)^2\n"
    "                           window best, then the best of its +-1 steps; --motion pyramid then searches one level less)\n"
    "  --hole-reach N           Reach of the compensated interpolator's hole fill (default: the 16 px walk; 1..255: a fill plane\n"
    "                           of two scans gives every hole the nearest vector within N px along each axis, at a cost\n"
    "                           that does not grow with N -- for the wide holes behind fast objects).  Needs --interpolator\n"
    "                           compensated; not with --generation extrapolate\n"
    "  --subpel-vectors R       Quarter-pixel vectors for the compensated interpolator (default -1: off; 0..2: the final integer\n"
    "                           field is refined to quarter pixels over each pixel's (2R+1)^2 window and the interpolation carries\n"
    "                           the fraction -- for content that moves by fractions of a pixel per frame).  Needs --interpolator\n"
    "                           compensated; not with --generation extrapolate, --bidirectional, --protect-static, --hole-reach\n"
    "                           or --ranks\n"
    "  --sharpen S              Contrast-limited sharpening of every presented frame, real and generated alike (default 0: off;\n"
    "                           1..64: strength in 64ths of the classic 5-point kernel, each pixel kept within the range of\n"
    "                           itself and its four neighbours).  Applied to a copy just before the read-back: motion, masks and\n"
    "                           cut detection see the unsharpened frames.  --evaluate does not sharpen\n"
    "  --scale-filter F         Filter of the scale to the output size: reference (default: the reference's six Lanczos-3 taps at\n"
    "                           every ratio), or nearest, bilinear, catmull-rom, mitchell, lanczos2, lanczos3 -- these widen with\n"
    "                           the ratio where the output is smaller than the input (anti-aliased downscaling); at most 64 taps\n"
    "                           per sample, which Lanczos-3 reaches at 10.6 : 1\n"
    "  --evaluate               Measure instead of presenting: source frames 0, 2, 4, ... are the stream, 1, 3, 5, ... are\n"
    "                           held out; each pair's frame at 0.5 is generated under the options above and compared on the\n"
    "                           GPU, at the output size, with the frame held out -- as is the pair's first frame, shown\n"
    "                           again.  The report gains \"evaluation\" (PSNR, error quantiles, differing pixels of both).\n"
    "                           With --generation extrapolate frames 2k and 2k + 1 predict frame 2k + 2, one interval ahead,\n"
    "                           and the yardstick is frame 2k + 1 shown again; the same frames are read, the same keys reported.\n"
    "                           Needs --frames >= 3; not with --ranks, --factors, --no-interpolation, --output-raw,\n"
    "                           --dump-dir or --replay\n"
    "  --frames N               Number of input frames to process (default: 10)\n"
    "  --device N               HIP device ordinal (default: 0)\n"
    "  --dump-dir DIR           Write every presented frame to DIR as raw RGBA8\n"
    "  --input-raw FILE         Read input frames (raw, tightly packed, back to back) from FILE, '-' = stdin\n"
    "  --output-raw FILE        Append every presented frame (raw) to FILE, '-' = stdout\n"
    "  --input-format rgba|nv12   What --input-raw holds (default rgba).  nv12: width*height bytes of luma, then width*height/2\n"
    "                           bytes of (Cb, Cr) pairs; 1.5 bytes per pixel are uploaded and converted on the GPU.  Needs\n"
    "                           --input-raw and even sizes; not with --ranks or --evaluate\n"
    "  --output-format rgba|nv12  What --output-raw and --dump-dir receive (default rgba).  nv12: every presented frame is\n"
    "                           converted on the GPU and 1.5 bytes per pixel are read back.  Even sizes; not with --ranks or --evaluate\n"
    "  --yuv-matrix 601|709     Colour matrix of both conversions (default 709)\n"
    "  --yuv-range limited|full Range of both conversions (default limited: luma 16..235, chroma 16..240)\n"
    "  --chroma replicate|left  Chroma siting of both conversions (default left: MPEG-2, co-sited with the even columns;\n"
    "                           replicate: each pair stands for its 2 x 2 pixels)\n"
    "  --replay N               Produce the source's first N frames once, before the clock starts, and play them back in rotation\n"
    "                           (the host's frame synthesis, 5 ms per 1080p frame, then does not bound the loop)\n"
    "  --present-null           The presenter looks at no pixel (default: a strided checksum over every presented frame)\n"
    "  --sync-present           Wait for each call's own frames (reference behaviour) instead of pipelining\n"
    "  --quiet                  Only warnings and errors\n";

namespace {
// The names of a Name row stand in the order of the library's constants: the enums of include/linuxfg_hip.h count from 0.
static_assert(LFG_ESTIMATOR_PYRAMID == 1 && LFG_SEMANTICS_INTENDED == 1 && LFG_INTERPOLATOR_COMPENSATED == 1 && LFG_GENERATION_EXTRAPOLATE == 1 &&
              LFG_YUV_BT709 == 1 && LFG_YUV_FULL == 1 && LFG_CHROMA_LEFT == 1 && LFG_FILTER_NEAREST == 0 && LFG_FILTER_LANCZOS3 == 5, "name order");
const char kFormats[] = "rgba|nv12";
const char kScaleFilters[] = "reference|nearest|bilinear|catmull-rom|mitchell|lanczos2|lanczos3";   // -1, then the lfg_filter values

bool SetFactors(Options& o, long, const char* list) {
    o.factors.clear();
    for (const char* p = list; *p;) {
        char* end = nullptr;
        o.factors.push_back(std::strtof(p, &end));
        if (end == p) return false;
        p = *end == ',' ? end + 1 : end;
    }
    return true;
}

// The `index`-th of `names`, which | separates; "" past the last.
std::string NameAt(const char* names, long index) {
    for (const char* p = names;; ++p) {
        const size_t length = strcspn(p, "|");
        if (index-- == 0) return std::string(p, length);
        p += length;
        if (!*p) return "";
    }
}

std::string Format(const char* format, ...) {
    va_list args, again;
    va_start(args, format);
    va_copy(again, args);
    std::string text((size_t)vsnprintf(nullptr, 0, format, args), '\0');
    vsnprintf(&text[0], text.size() + 1, format, again);       // (a std::string owns the NUL at size(), which this writes again)
    va_end(again);
    va_end(args);
    return text;
}
}  // namespace

#define SET(statement) [](Options& o, long n, const char* s) { (void)o; (void)n; (void)s; statement; return true; }
const OptionRow kOptionRows[] = {
    {OptionRow::Flag, "--help", 0, 0, nullptr, SET(o.help = true)},
    {OptionRow::Lenient, "--input-width", 0, 0, nullptr, SET(o.config.inputWidth = (uint32_t)n)},
    {OptionRow::Lenient, "--input-height", 0, 0, nullptr, SET(o.config.inputHeight = (uint32_t)n)},
    {OptionRow::Lenient, "--output-width", 0, 0, nullptr, SET(o.config.outputWidth = (uint32_t)n)},
    {OptionRow::Lenient, "--output-height", 0, 0, nullptr, SET(o.config.outputHeight = (uint32_t)n)},
    {OptionRow::Lenient, "--target-fps", 0, 0, nullptr, SET(o.config.targetFps = (uint32_t)n)},
    {OptionRow::Flag, "--no-interpolation", 0, 0, nullptr, SET(o.config.enableInterpolation = false)},
    {OptionRow::Text, "--interpolation-factor", 0, 0, nullptr, SET(o.config.interpolationFactor = (float)std::atof(s))},
    {OptionRow::Text, "--factors", 0, 0, "list", SetFactors},
    {OptionRow::Lenient, "--in-flight", 0, 0, nullptr, SET(o.inFlight = (int)n)},
    {OptionRow::Lenient, "--ranks", 0, 0, nullptr, SET(o.ranks = (int)n)},
    {OptionRow::Lenient, "--rank", 0, 0, nullptr, SET(o.rank = (int)n)},
    {OptionRow::Text, "--comm-file", 0, 0, nullptr, SET(o.commFile = s)},
    {OptionRow::Text, "--comm-nonce", 0, 0, nullptr, SET(o.commNonce = strtoull(s, nullptr, 0))},
    {OptionRow::Name, "--motion", 0, 0, "full|pyramid", SET(o.route.estimator = (int)n)},
    {OptionRow::Name, "--semantics", 0, 0, "reference|intended", SET(o.route.semantics = (int)n)},
    {OptionRow::Name, "--interpolator", 0, 0, "shader|compensated", SET(o.route.interpolator = (int)n)},
    {OptionRow::Name, "--generation", 0, 0, "interpolate|extrapolate", SET(o.route.generation = (int)n)},
    {OptionRow::Whole, "--refine-vectors", -1, 2, "-1, 0, 1 or 2", SET(o.route.refineRadius = (int)n)},
    {OptionRow::Whole, "--cut-threshold", -1, 1000, "-1, or 0 to 1000", SET(o.route.cutThreshold = (int)n)},
    {OptionRow::Whole, "--protect-static", -1, 1020, "-1, or 0 to 1020", SET(o.route.staticTolerance = (int)n)},
    {OptionRow::Whole, "--bidirectional", -1, 64, "-1, or 0 to 64", SET(o.route.bidirectional = (int)n)},
    {OptionRow::Whole, "--half-res-motion", -1, 2, "-1, 0, 1 or 2", SET(o.route.halfResMotion = (int)n)},
    {OptionRow::Whole, "--hole-reach", 1, LFG_HOLE_REACH_MAX, "1 to 255", SET(o.route.holeReach = (int)n)},
    {OptionRow::Whole, "--subpel-vectors", -1, 2, "-1, 0, 1 or 2", SET(o.route.subpelVectors = (int)n)},
    {OptionRow::Whole, "--sharpen", 0, 64, "0 to 64", SET(o.config.sharpen = (uint32_t)n)},
    {OptionRow::Name, "--scale-filter", 0, 0, kScaleFilters, SET(o.config.scaleFilter = (int)n - 1)},
    {OptionRow::Flag, "--evaluate", 0, 0, nullptr, SET(o.evaluate = true)},
    {OptionRow::Lenient, "--frames", 0, 0, nullptr, SET(o.frames = (int)n)},
    {OptionRow::Lenient, "--device", 0, 0, nullptr, SET(o.device = (int)n)},
    {OptionRow::Text, "--dump-dir", 0, 0, nullptr, SET(o.dumpDir = s)},
    {OptionRow::Text, "--input-raw", 0, 0, nullptr, SET(o.inputRaw = s)},
    {OptionRow::Text, "--output-raw", 0, 0, nullptr, SET(o.outputRaw = s)},
    {OptionRow::Name, "--input-format", 0, 0, kFormats, SET(o.inputNv12 = n == 1)},
    {OptionRow::Name, "--output-format", 0, 0, kFormats, SET(o.outputNv12 = n == 1)},
    {OptionRow::Name, "--yuv-matrix", 0, 0, "601|709", SET(o.yuv.matrix = (int)n)},
    {OptionRow::Name, "--yuv-range", 0, 0, "limited|full", SET(o.yuv.range = (int)n)},
    {OptionRow::Name, "--chroma", 0, 0, "replicate|left", SET(o.yuv.siting = (int)n)},
    {OptionRow::Flag, "--sync-present", 0, 0, nullptr, SET(o.syncPresent = true)},
    {OptionRow::Lenient, "--replay", 0, 0, nullptr, SET(o.replay = (int)n)},
    {OptionRow::Flag, "--present-null", 0, 0, nullptr, SET(o.presentNull = true)},
    {OptionRow::Flag, "--quiet", 0, 0, nullptr, SET(o.quiet = true)},
};
#undef SET
const size_t kOptionRowCount = sizeof kOptionRows / sizeof kOptionRows[0];

std::string ParseOptions(int argc, const char* const* argv, Options& o) {
    if (const char* nonce = getenv("LFG_COMM_NONCE")) o.commNonce = strtoull(nonce, nullptr, 0);
    for (int i = 1; i < argc; i++) {
        const OptionRow* row = nullptr;
        for (size_t r = 0; r < kOptionRowCount && !row; ++r)
            if (strcmp(argv[i], kOptionRows[r].name) == 0 && (kOptionRows[r].kind == OptionRow::Flag || i + 1 < argc)) row = &kOptionRows[r];
        if (!row) {
            char* end = nullptr;
            o.stream = (uint32_t)std::strtoul(argv[i], &end, 0);
            if (*end != '\0') return "Invalid stream index";
            continue;
        }
        const char* value = row->kind == OptionRow::Flag ? nullptr : argv[++i];
        long n = 0;
        bool ok = true;
        if (row->kind == OptionRow::Lenient) n = std::atoi(value);
        if (row->kind == OptionRow::Whole) {
            char* end = nullptr;
            n = strtol(value, &end, 10);
            ok = end != value && *end == '\0' && n >= row->lo && n <= row->hi;
        }
        if (row->kind == OptionRow::Name) {
            std::string name;                         // the first that is the value, or "" past the last
            for (n = 0; !(name = NameAt(row->bracket, n)).empty() && name != value;) ++n;
            ok = !name.empty();
        }
        if (!ok || !row->set(o, n, value))
            return std::string("Invalid ") + row->name + (row->kind == OptionRow::Text ? std::string(" ") + row->bracket : " (" + std::string(row->bracket) + ")");
        if (o.help) return "";
    }
    ScalerConfig& config = o.config;
    if (config.inputWidth == 0) config.inputWidth = 1920;
    if (config.inputHeight == 0) config.inputHeight = 1080;
    // Output size: as src/main.cpp:76-90 (keep the aspect ratio when only one side is given).
    if (config.outputWidth == 0 || config.outputHeight == 0) {
        if (config.outputHeight != 0) {
            float scale = (float)config.outputHeight / config.inputHeight;
            config.outputWidth = static_cast<uint32_t>(config.inputWidth * scale);
        } else if (config.outputWidth != 0) {
            float scale = (float)config.outputWidth / config.inputWidth;
            config.outputHeight = static_cast<uint32_t>(config.inputHeight * scale);
        } else {
            config.outputWidth = config.inputWidth;
            config.outputHeight = config.inputHeight;
        }
    }
    return "";
}

std::string CheckOptions(const Options& o, const std::function<bool(int, uint32_t, uint32_t)>& tapsFit) {
    const ScalerConfig& config = o.config;
    const Route& r = o.route;
    const bool compensated = r.interpolator == LFG_INTERPOLATOR_COMPENSATED, extrapolate = r.generation == LFG_GENERATION_EXTRAPOLATE;
    if (o.inputNv12 || o.outputNv12) {
        const std::string which = o.inputNv12 ? "--input-format nv12" : "--output-format nv12";
        if (o.ranks > 0 || o.evaluate) return which + " cannot be combined with " + (o.ranks > 0 ? "--ranks" : "--evaluate");
        if (o.inputNv12 && o.inputRaw.empty()) return "--input-format nv12 needs --input-raw (the synthetic source makes RGBA8)";
        if ((o.inputNv12 && (config.inputWidth % 2 || config.inputHeight % 2)) || (o.outputNv12 && (config.outputWidth % 2 || config.outputHeight % 2)))
            return "NV12 needs an even width and height";
    }
    if (config.scaleFilter >= 0) {
        for (int axis = 0; axis < 2; ++axis) {
            const uint32_t in = axis ? config.inputHeight : config.inputWidth, out = axis ? config.outputHeight : config.outputWidth;
            if (!tapsFit(config.scaleFilter, in, out))
                return "--scale-filter " + NameAt(kScaleFilters, config.scaleFilter + 1) + " cannot scale " + std::to_string(in) + " to " + std::to_string(out) +
                       " (more than 64 taps per sample)";
        }
    }
    if (extrapolate) {
        if (!compensated) return "--generation extrapolate needs --interpolator compensated";
        if (o.ranks > 0) return "--generation extrapolate cannot be combined with --ranks";
    }
    if (r.holeReach >= 1) {
        if (!compensated) return "--hole-reach needs --interpolator compensated";
        if (extrapolate) return "--hole-reach cannot be combined with --generation extrapolate";
    }
    if (r.subpelVectors >= 0) {
        const char* clash = !compensated ? "--interpolator shader" : extrapolate ? "--generation extrapolate" : r.bidirectional >= 0 ? "--bidirectional"
                          : r.staticTolerance >= 0 ? "--protect-static" : r.holeReach >= 1 ? "--hole-reach" : o.ranks > 0 ? "--ranks" : nullptr;
        if (clash) return std::string("--subpel-vectors cannot be combined with ") + clash;
    }
    if (o.evaluate) {
        const char* clash = o.ranks > 0 ? "--ranks" : !o.factors.empty() ? "--factors" : !config.enableInterpolation ? "--no-interpolation"
                          : !o.outputRaw.empty() ? "--output-raw" : !o.dumpDir.empty() ? "--dump-dir" : o.replay > 0 ? "--replay" : nullptr;
        if (clash) return std::string("--evaluate cannot be combined with ") + clash;
        if (o.frames < 3) return "--evaluate needs --frames of 3 or more";
    }
    return "";
}

std::string ReportLine(const Options& o, const ReportCounters& c) {
    const bool shown = !o.evaluate;                    // --evaluate presents nothing, on one lane, from and to RGBA8, unsharpened
    const Route& r = o.route;
    std::string line = Format("{\"input_frames\": %d, \"presented\": %llu, \"interpolated\": %llu, \"cuts\": %llu, \"seconds\": %.4f, "
                              "\"presented_fps\": %.2f, \"checksum\": %llu, \"pipelined\": %s, \"replay\": %d, \"present_null\": %s, \"in_flight\": %d, "
                              "\"input_format\": \"%s\", \"output_format\": \"%s\", \"protect_static\": %d, ",
                              o.frames, (unsigned long long)(shown ? c.presented : 0), (unsigned long long)c.generated, (unsigned long long)(shown ? c.cuts : 0),
                              c.seconds, shown ? c.presented / c.seconds : 0.0, (unsigned long long)(shown ? c.checksum : 0),
                              shown && !o.syncPresent ? "true" : "false", shown ? o.replay : 0, o.presentNull ? "true" : "false", shown ? o.inFlight : 1,
                              shown && o.inputNv12 ? "nv12" : "rgba", shown && o.outputNv12 ? "nv12" : "rgba", r.staticTolerance);
    const auto field = [&line](const char* key, int value, int from) { if (value >= from) line += Format("\"%s\": %d, ", key, value); };
    if (shown) field("sharpen", (int)o.config.sharpen, 1);
    if (o.config.scaleFilter >= 0) line += "\"scale_filter\": \"" + NameAt(kScaleFilters, o.config.scaleFilter + 1) + "\", ";
    field("bidirectional", r.bidirectional, 0);
    field("half_res_motion", r.halfResMotion, 0);
    field("hole_reach", r.holeReach, 1);
    field("subpel_vectors", r.subpelVectors, 0);
    if (!shown) return line + "\"note\": \"nothing is presented: every second source frame is held out and compared on the GPU\", \"evaluation\": " + c.evaluation + "}\n";
    return line + "\"note\": \"includes " + (o.replay > 0 ? "one memcpy per input frame into the staging slot" : "host frame synthesis") + ", PCIe upload and readback\"}\n";
}
