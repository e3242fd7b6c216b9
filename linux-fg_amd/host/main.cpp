// lfg_host -- headless counterpart of the reference's CLI (src/main.cpp:21-144): same option names
// and the same derivation of the output size; the X11 window id is replaced by a synthetic stream
// index and the paced SDL loop by a fixed number of frames run flat out.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "evaluate.hpp"
#include "scaler.hpp"

static void PrintUsage() {
    std::cout << "Usage: lfg_host [options] [stream-index]\n"
              << "Options:\n"
              << "  --help                   Show this help message\n"
              << "  --input-width WIDTH      Input width (default: 1920)\n"
              << "  --input-height HEIGHT    Input height (default: 1080)\n"
              << "  --output-width WIDTH     Output width\n"
              << "  --output-height HEIGHT   Output height\n"
              << "  --target-fps FPS         Accepted for compatibility; frames are not paced\n"
              << "  --no-interpolation       Disable frame interpolation\n"
              << "  --interpolation-factor F Interpolation blend factor (0.0-1.0, default: 0.5)\n"
              << "  --factors A,B,...        Several generated frames per pair, in presentation order (e.g. 0.25,0.5,0.75\n"
              << "                           for 60 -> 240 fps); motion runs once per pair\n"
              << "  --in-flight N            Frames in flight on the GPU, 1..3 (default 2): a frame's upscale and first motion units\n"
              << "                           run while the previous frame's last long units finish; same frames, same order\n"
              << "  --ranks N --rank R --comm-file FILE\n"
              << "                           One process per GPU (BASELINE config 4): the batch shares its previous frame\n"
              << "                           (synthetic stream 0, captured on rank 0, broadcast over RCCL per frame); each\n"
              << "                           rank's current frames are its own stream.  FILE carries the communicator id.\n"
              << "  --comm-nonce N           A number the launcher gives every rank of ONE run (default: LFG_COMM_NONCE, else 0; more than one rank needs a non-zero one): an\n"
              << "                           id file left behind by another run is then never joined\n"
              << "  --motion full|pyramid    Motion estimator of the generated frames (default full: the reference's +-16 search;\n"
              << "                           pyramid: coarse-to-fine, +-70 px at a cost independent of the content)\n"
              << "  --semantics reference|intended  Arithmetic of motion and interpolation (default reference: the shaders as\n"
              << "                           written; intended: vectors displace by pixels -- what vectors longer than 1 px need)\n"
              << "  --interpolator shader|compensated  Interpolation of the generated frames (default shader: the reference's;\n"
              << "                           compensated: vectors projected to the frame's time, holes filled; wants --semantics intended)\n"
              << "  --generation interpolate|extrapolate  Where the generated frames lie (default interpolate: between the last two real\n"
              << "                           frames, the newest one held back until they are shown; extrapolate: AHEAD of the newest real\n"
              << "                           frame, which is presented as it arrives, each factor read as the fraction of an interval\n"
              << "                           ahead).  extrapolate needs --interpolator compensated and is not available with --ranks\n"
              << "  --refine-vectors R       Per-pixel vector refinement between motion and interpolation (default -1: off;\n"
              << "                           0..2: each pixel takes the nearby vector that fits its (2R+1)^2 window best)\n"
              << "  --cut-threshold P        Scene-cut detection (default -1: off; 0..1000: a pair of which fewer than P pixels per\n"
              << "                           thousand match under its vectors shows a source frame instead of a generated one)\n"
              << "  --protect-static T       Static-overlay protection of the compensated interpolator (default -1: off; 0..1020: pixels\n"
              << "                           whose four channels differ by at most T in sum between the pair's frames stay where they\n"
              << "                           are -- a HUD, a crosshair, text; no effect with --interpolator shader)\n"
              << "  --bidirectional T        Bidirectional compensated interpolation (default -1: off; 0..64: the pair is measured both ways,\n"
              << "                           a vector projects only where the two fields agree within T in L1, and both frames' grids\n"
              << "                           project; doubles the motion stage.  No effect with --interpolator shader, --generation\n"
              << "                           extrapolate or --protect-static)\n"
              << "  --half-res-motion R      Half-resolution motion (default -1: off; 0..2: the estimator runs on both frames halved and\n"
              << "                           each pixel takes the doubled vector of the 3 x 3 coarse neighbours that fits its (2R+1)^2\n"
              << "                           window best, then the best of its +-1 steps; --motion pyramid then searches one level less)\n"
              << "  --hole-reach N           Reach of the compensated interpolator's hole fill (default: the 16 px walk; 1..255: a fill plane\n"
              << "                           of two scans gives every hole the nearest vector within N px along each axis, at a cost\n"
              << "                           that does not grow with N -- for the wide holes behind fast objects).  Needs --interpolator\n"
              << "                           compensated; not with --generation extrapolate\n"
              << "  --subpel-vectors R       Quarter-pixel vectors for the compensated interpolator (default -1: off; 0..2: the final integer\n"
              << "                           field is refined to quarter pixels over each pixel's (2R+1)^2 window and the interpolation carries\n"
              << "                           the fraction -- for content that moves by fractions of a pixel per frame).  Needs --interpolator\n"
              << "                           compensated; not with --generation extrapolate, --bidirectional, --protect-static, --hole-reach\n"
              << "                           or --ranks\n"
              << "  --sharpen S              Contrast-limited sharpening of every presented frame, real and generated alike (default 0: off;\n"
              << "                           1..64: strength in 64ths of the classic 5-point kernel, each pixel kept within the range of\n"
              << "                           itself and its four neighbours).  Applied to a copy just before the read-back: motion, masks and\n"
              << "                           cut detection see the unsharpened frames.  --evaluate does not sharpen\n"
              << "  --scale-filter F         Filter of the scale to the output size: reference (default: the reference's six Lanczos-3 taps at\n"
              << "                           every ratio), or nearest, bilinear, catmull-rom, mitchell, lanczos2, lanczos3 -- these widen with\n"
              << "                           the ratio where the output is smaller than the input (anti-aliased downscaling); at most 64 taps\n"
              << "                           per sample, which Lanczos-3 reaches at 10.6 : 1\n"
              << "  --evaluate               Measure instead of presenting: source frames 0, 2, 4, ... are the stream, 1, 3, 5, ... are\n"
              << "                           held out; each pair's frame at 0.5 is generated under the options above and compared on the\n"
              << "                           GPU, at the output size, with the frame held out -- as is the pair's first frame, shown\n"
              << "                           again.  The report gains \"evaluation\" (PSNR, error quantiles, differing pixels of both).\n"
              << "                           With --generation extrapolate frames 2k and 2k + 1 predict frame 2k + 2, one interval ahead,\n"
              << "                           and the yardstick is frame 2k + 1 shown again; the same frames are read, the same keys reported.\n"
              << "                           Needs --frames >= 3; not with --ranks, --factors, --no-interpolation, --output-raw,\n"
              << "                           --dump-dir or --replay\n"
              << "  --frames N               Number of input frames to process (default: 10)\n"
              << "  --device N               HIP device ordinal (default: 0)\n"
              << "  --dump-dir DIR           Write every presented frame to DIR as raw RGBA8\n"
              << "  --input-raw FILE         Read input frames (raw, tightly packed, back to back) from FILE, '-' = stdin\n"
              << "  --output-raw FILE        Append every presented frame (raw) to FILE, '-' = stdout\n"
              << "  --input-format rgba|nv12   What --input-raw holds (default rgba).  nv12: width*height bytes of luma, then width*height/2\n"
              << "                           bytes of (Cb, Cr) pairs; 1.5 bytes per pixel are uploaded and converted on the GPU.  Needs\n"
              << "                           --input-raw and even sizes; not with --ranks or --evaluate\n"
              << "  --output-format rgba|nv12  What --output-raw and --dump-dir receive (default rgba).  nv12: every presented frame is\n"
              << "                           converted on the GPU and 1.5 bytes per pixel are read back.  Even sizes; not with --ranks or --evaluate\n"
              << "  --yuv-matrix 601|709     Colour matrix of both conversions (default 709)\n"
              << "  --yuv-range limited|full Range of both conversions (default limited: luma 16..235, chroma 16..240)\n"
              << "  --chroma replicate|left  Chroma siting of both conversions (default left: MPEG-2, co-sited with the even columns;\n"
              << "                           replicate: each pair stands for its 2 x 2 pixels)\n"
              << "  --replay N               Produce the source's first N frames once, before the clock starts, and play them back in rotation\n"
              << "                           (the host's frame synthesis, 5 ms per 1080p frame, then does not bound the loop)\n"
              << "  --present-null           The presenter looks at no pixel (default: a strided checksum over every presented frame)\n"
              << "  --sync-present           Wait for each call's own frames (reference behaviour) instead of pipelining\n"
              << "  --quiet                  Only warnings and errors\n";
}

// --scale-filter: the names of LFG_FILTER_NEAREST .. LFG_FILTER_LANCZOS3, in the enum's order
static const char* const kScaleFilterNames[6] = {"nearest", "bilinear", "catmull-rom", "mitchell", "lanczos2", "lanczos3"};

int main(int argc, char* argv[]) {
    // (HIP's default of four hardware queues is one short of three lanes + a copy stream + a communication stream: streams that
    //  share a queue run in turn.  Before the first HIP call; an explicit setting wins.  INTEGRATION.md, "Hardware queues".)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    ScalerConfig config;
    config.enableInterpolation = true;
    config.interpolationFactor = 0.5f;
    config.targetFps = 60;
    uint32_t stream = 0;
    int frames = 10, device = 0;
    std::string dumpDir, inputRaw, outputRaw, commFile;
    int ranks = 0, rank = 0, inFlight = 2;
    int estimator = LFG_ESTIMATOR_FULL_SEARCH, semantics = LFG_SEMANTICS_REFERENCE, interpolator = LFG_INTERPOLATOR_SHADER, refineRadius = -1, cutThreshold = -1, staticTolerance = -1,
        generation = LFG_GENERATION_INTERPOLATE, bidirectional = -1, halfResMotion = -1, holeReach = -1;
    unsigned long long commNonce = getenv("LFG_COMM_NONCE") ? strtoull(getenv("LFG_COMM_NONCE"), nullptr, 0) : 0ull;
    std::vector<float> factors;
    bool syncPresent = false, presentNull = false, evaluate = false, inputNv12 = false, outputNv12 = false;
    Scaler::YuvModes yuv;
    int replay = 0;

    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--help") == 0) { PrintUsage(); return 0; }
        else if (strcmp(argv[i], "--input-width") == 0 && i + 1 < argc) config.inputWidth = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--input-height") == 0 && i + 1 < argc) config.inputHeight = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--output-width") == 0 && i + 1 < argc) config.outputWidth = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--output-height") == 0 && i + 1 < argc) config.outputHeight = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--target-fps") == 0 && i + 1 < argc) config.targetFps = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--no-interpolation") == 0) config.enableInterpolation = false;
        else if (strcmp(argv[i], "--interpolation-factor") == 0 && i + 1 < argc) config.interpolationFactor = (float)std::atof(argv[++i]);
        else if (strcmp(argv[i], "--factors") == 0 && i + 1 < argc) {
            factors.clear();
            for (const char* p = argv[++i]; *p;) {
                char* end = nullptr;
                factors.push_back(std::strtof(p, &end));
                if (end == p) { LOG_ERROR("Invalid --factors list"); return 1; }
                p = *end == ',' ? end + 1 : end;
            }
        }
        else if (strcmp(argv[i], "--in-flight") == 0 && i + 1 < argc) inFlight = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--ranks") == 0 && i + 1 < argc) ranks = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--rank") == 0 && i + 1 < argc) rank = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--comm-file") == 0 && i + 1 < argc) commFile = argv[++i];
        else if (strcmp(argv[i], "--comm-nonce") == 0 && i + 1 < argc) commNonce = strtoull(argv[++i], nullptr, 0);
        else if (strcmp(argv[i], "--motion") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "full") == 0) estimator = LFG_ESTIMATOR_FULL_SEARCH;
            else if (strcmp(m, "pyramid") == 0) estimator = LFG_ESTIMATOR_PYRAMID;
            else { LOG_ERROR("Invalid --motion (full|pyramid)"); return 1; }
        }
        else if (strcmp(argv[i], "--semantics") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "reference") == 0) semantics = LFG_SEMANTICS_REFERENCE;
            else if (strcmp(m, "intended") == 0) semantics = LFG_SEMANTICS_INTENDED;
            else { LOG_ERROR("Invalid --semantics (reference|intended)"); return 1; }
        }
        else if (strcmp(argv[i], "--interpolator") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "shader") == 0) interpolator = LFG_INTERPOLATOR_SHADER;
            else if (strcmp(m, "compensated") == 0) interpolator = LFG_INTERPOLATOR_COMPENSATED;
            else { LOG_ERROR("Invalid --interpolator (shader|compensated)"); return 1; }
        }
        else if (strcmp(argv[i], "--generation") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "interpolate") == 0) generation = LFG_GENERATION_INTERPOLATE;
            else if (strcmp(m, "extrapolate") == 0) generation = LFG_GENERATION_EXTRAPOLATE;
            else { LOG_ERROR("Invalid --generation (interpolate|extrapolate)"); return 1; }
        }
        else if (strcmp(argv[i], "--refine-vectors") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long r = strtol(argv[++i], &end, 10);
            if (!end || *end != '\0' || r < -1 || r > 2) { LOG_ERROR("Invalid --refine-vectors (-1, 0, 1 or 2)"); return 1; }
            refineRadius = (int)r;
        }
        else if (strcmp(argv[i], "--cut-threshold") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long p = strtol(argv[++i], &end, 10);
            if (!end || *end != '\0' || p < -1 || p > 1000) { LOG_ERROR("Invalid --cut-threshold (-1, or 0 to 1000)"); return 1; }
            cutThreshold = (int)p;
        }
        else if (strcmp(argv[i], "--protect-static") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long t = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end != '\0' || t < -1 || t > 1020) { LOG_ERROR("Invalid --protect-static (-1, or 0 to 1020)"); return 1; }
            staticTolerance = (int)t;
        }
        else if (strcmp(argv[i], "--bidirectional") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long t = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end != '\0' || t < -1 || t > 64) { LOG_ERROR("Invalid --bidirectional (-1, or 0 to 64)"); return 1; }
            bidirectional = (int)t;
        }
        else if (strcmp(argv[i], "--half-res-motion") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long r = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end != '\0' || r < -1 || r > 2) { LOG_ERROR("Invalid --half-res-motion (-1, 0, 1 or 2)"); return 1; }
            halfResMotion = (int)r;
        }
        else if (strcmp(argv[i], "--hole-reach") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long n = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end != '\0' || n < 1 || n > LFG_HOLE_REACH_MAX) { LOG_ERROR("Invalid --hole-reach (1 to 255)"); return 1; }
            holeReach = (int)n;
        }
        else if (strcmp(argv[i], "--subpel-vectors") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long r = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end != '\0' || r < -1 || r > 2) { LOG_ERROR("Invalid --subpel-vectors (-1, 0, 1 or 2)"); return 1; }
            config.subpelVectors = (int)r;
        }
        else if (strcmp(argv[i], "--sharpen") == 0 && i + 1 < argc) {
            char* end = nullptr;
            const long v = strtol(argv[++i], &end, 10);
            if (!end || end == argv[i] || *end != '\0' || v < 0 || v > 64) { LOG_ERROR("Invalid --sharpen (0 to 64)"); return 1; }
            config.sharpen = (uint32_t)v;
        }
        else if (strcmp(argv[i], "--scale-filter") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            config.scaleFilter = -2;
            if (strcmp(m, "reference") == 0) config.scaleFilter = -1;
            for (int f = 0; f < 6; ++f)
                if (strcmp(m, kScaleFilterNames[f]) == 0) config.scaleFilter = f;
            if (config.scaleFilter == -2) { LOG_ERROR("Invalid --scale-filter (reference|nearest|bilinear|catmull-rom|mitchell|lanczos2|lanczos3)"); return 1; }
        }
        else if (strcmp(argv[i], "--evaluate") == 0) evaluate = true;
        else if (strcmp(argv[i], "--frames") == 0 && i + 1 < argc) frames = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--device") == 0 && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--dump-dir") == 0 && i + 1 < argc) dumpDir = argv[++i];
        else if (strcmp(argv[i], "--input-raw") == 0 && i + 1 < argc) inputRaw = argv[++i];
        else if (strcmp(argv[i], "--output-raw") == 0 && i + 1 < argc) outputRaw = argv[++i];
        else if ((strcmp(argv[i], "--input-format") == 0 || strcmp(argv[i], "--output-format") == 0) && i + 1 < argc) {
            bool& nv12 = strcmp(argv[i], "--input-format") == 0 ? inputNv12 : outputNv12;
            const char* m = argv[++i];
            if (strcmp(m, "rgba") == 0) nv12 = false;
            else if (strcmp(m, "nv12") == 0) nv12 = true;
            else { LOG_ERROR("Invalid ", argv[i - 1], " (rgba|nv12)"); return 1; }
        }
        else if (strcmp(argv[i], "--yuv-matrix") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "601") == 0) yuv.matrix = LFG_YUV_BT601;
            else if (strcmp(m, "709") == 0) yuv.matrix = LFG_YUV_BT709;
            else { LOG_ERROR("Invalid --yuv-matrix (601|709)"); return 1; }
        }
        else if (strcmp(argv[i], "--yuv-range") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "limited") == 0) yuv.range = LFG_YUV_LIMITED;
            else if (strcmp(m, "full") == 0) yuv.range = LFG_YUV_FULL;
            else { LOG_ERROR("Invalid --yuv-range (limited|full)"); return 1; }
        }
        else if (strcmp(argv[i], "--chroma") == 0 && i + 1 < argc) {
            const char* m = argv[++i];
            if (strcmp(m, "replicate") == 0) yuv.siting = LFG_CHROMA_REPLICATE;
            else if (strcmp(m, "left") == 0) yuv.siting = LFG_CHROMA_LEFT;
            else { LOG_ERROR("Invalid --chroma (replicate|left)"); return 1; }
        }
        else if (strcmp(argv[i], "--sync-present") == 0) syncPresent = true;
        else if (strcmp(argv[i], "--replay") == 0 && i + 1 < argc) replay = std::atoi(argv[++i]);
        else if (strcmp(argv[i], "--present-null") == 0) presentNull = true;
        else if (strcmp(argv[i], "--quiet") == 0) Logger::Get().SetMinLevel(Logger::Level::WARNING);
        else {
            char* endPtr;
            stream = (uint32_t)std::strtoul(argv[i], &endPtr, 0);
            if (*endPtr != '\0') { LOG_ERROR("Invalid stream index"); return 1; }
        }
    }
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

    if (inputNv12 || outputNv12) {                              // before a context is made
        const char* which = inputNv12 ? "--input-format nv12" : "--output-format nv12";
        if (ranks > 0 || evaluate) { LOG_ERROR(which, " cannot be combined with ", ranks > 0 ? "--ranks" : "--evaluate"); return 2; }
        if (inputNv12 && inputRaw.empty()) { LOG_ERROR("--input-format nv12 needs --input-raw (the synthetic source makes RGBA8)"); return 2; }
        if ((inputNv12 && (config.inputWidth % 2 || config.inputHeight % 2)) || (outputNv12 && (config.outputWidth % 2 || config.outputHeight % 2))) {
            LOG_ERROR("NV12 needs an even width and height");
            return 2;
        }
    }
    if (config.scaleFilter >= 0) {                              // before a context is made: the tables are a host function
        for (int axis = 0; axis < 2; ++axis) {
            const uint32_t in = axis ? config.inputHeight : config.inputWidth, out = axis ? config.outputHeight : config.outputWidth;
            std::vector<int32_t> first(out);
            std::vector<uint32_t> count(out);
            std::vector<int16_t> weights((size_t)out * LFG_RESAMPLE_MAX_TAPS);
            if (lfg_resample_taps(config.scaleFilter, in, out, first.data(), count.data(), weights.data()) != LFG_OK) {
                LOG_ERROR("--scale-filter ", kScaleFilterNames[config.scaleFilter], " cannot scale ", in, " to ", out, " (more than 64 taps per sample)");
                return 2;
            }
        }
    }
    if (generation == LFG_GENERATION_EXTRAPOLATE) {            // before a context is made
        if (interpolator != LFG_INTERPOLATOR_COMPENSATED) { LOG_ERROR("--generation extrapolate needs --interpolator compensated"); return 2; }
        if (ranks > 0) { LOG_ERROR("--generation extrapolate cannot be combined with --ranks"); return 2; }
    }
    if (holeReach >= 1) {                                       // before a context is made
        if (interpolator != LFG_INTERPOLATOR_COMPENSATED) { LOG_ERROR("--hole-reach needs --interpolator compensated"); return 2; }
        if (generation == LFG_GENERATION_EXTRAPOLATE) { LOG_ERROR("--hole-reach cannot be combined with --generation extrapolate"); return 2; }
    }
    if (config.subpelVectors >= 0) {                            // before a context is made
        const char* clash = interpolator != LFG_INTERPOLATOR_COMPENSATED ? "--interpolator shader"
                          : generation == LFG_GENERATION_EXTRAPOLATE ? "--generation extrapolate" : bidirectional >= 0 ? "--bidirectional"
                          : staticTolerance >= 0 ? "--protect-static" : holeReach >= 1 ? "--hole-reach" : ranks > 0 ? "--ranks" : nullptr;
        if (clash) { LOG_ERROR("--subpel-vectors cannot be combined with ", clash); return 2; }
    }
    if (evaluate) {                                             // before a context is made
        const char* clash = ranks > 0 ? "--ranks" : !factors.empty() ? "--factors" : !config.enableInterpolation ? "--no-interpolation"
                          : !outputRaw.empty() ? "--output-raw" : !dumpDir.empty() ? "--dump-dir" : replay > 0 ? "--replay" : nullptr;
        if (clash) { LOG_ERROR("--evaluate cannot be combined with ", clash); return 2; }
        if (frames < 3) { LOG_ERROR("--evaluate needs --frames of 3 or more"); return 2; }
    }

    if (!HipContext::Get().Initialize(device)) { LOG_ERROR("Failed to initialize HIP"); return 1; }
    // (library settings, like --in-flight: ScalerConfig keeps the reference's fields)
    if (lfg_set_semantics(HipContext::Get().GetDevice(), semantics) != LFG_OK ||
        lfg_set_motion_estimator(HipContext::Get().GetDevice(), estimator) != LFG_OK ||
        lfg_set_interpolator(HipContext::Get().GetDevice(), interpolator, 48) != LFG_OK ||
        lfg_set_vector_refinement(HipContext::Get().GetDevice(), refineRadius) != LFG_OK ||
        lfg_set_cut_detection(HipContext::Get().GetDevice(), cutThreshold) != LFG_OK ||
        lfg_set_static_protection(HipContext::Get().GetDevice(), staticTolerance) != LFG_OK) {
        LOG_ERROR("Failed to set the motion options: ", lfg_last_error(HipContext::Get().GetDevice()));
        HipContext::Get().Cleanup();
        return 1;
    }
    if (!FrameManager::Get().Initialize(config.outputWidth, config.outputHeight) || !FrameManager::Get().SetGeneration(generation) ||
        !FrameManager::Get().SetBidirectional(bidirectional) || !FrameManager::Get().SetHalfResolutionMotion(halfResMotion) ||
        !FrameManager::Get().SetHoleReach(holeReach) || !FrameManager::Get().SetSubpixelVectors(config.subpelVectors)) {
        LOG_ERROR("Failed to initialize frame manager");
        HipContext::Get().Cleanup();
        return 1;
    }
    if (evaluate) {
        std::unique_ptr<FrameSource> source;
        if (!inputRaw.empty()) source = std::make_unique<RawFileCapture>(inputRaw);
        else source = std::make_unique<SyntheticCapture>(stream);
        EvaluationResult result;
        const bool ok = RunEvaluation(*source, config.inputWidth, config.inputHeight, config.outputWidth, config.outputHeight, frames, result,
                                      generation == LFG_GENERATION_EXTRAPOLATE, config.scaleFilter);
        source.reset();
        FrameManager::Get().Cleanup();
        HipContext::Get().Cleanup();
        if (!ok) { LOG_ERROR("Evaluation failed: ", Logger::Get().GetLastError()); return 1; }
        char filterField[136] = "";
        int used = 0;
        if (config.scaleFilter >= 0) used = snprintf(filterField, sizeof filterField, "\"scale_filter\": \"%s\", ", kScaleFilterNames[config.scaleFilter]);
        if (bidirectional >= 0) used += snprintf(filterField + used, sizeof filterField - (size_t)used, "\"bidirectional\": %d, ", bidirectional);
        if (halfResMotion >= 0) used += snprintf(filterField + used, sizeof filterField - (size_t)used, "\"half_res_motion\": %d, ", halfResMotion);
        if (holeReach >= 1) used += snprintf(filterField + used, sizeof filterField - (size_t)used, "\"hole_reach\": %d, ", holeReach);
        if (config.subpelVectors >= 0) snprintf(filterField + used, sizeof filterField - (size_t)used, "\"subpel_vectors\": %d, ", config.subpelVectors);
        printf("{\"input_frames\": %d, \"presented\": 0, \"interpolated\": %llu, \"cuts\": 0, \"seconds\": %.4f, "
               "\"presented_fps\": 0.00, \"checksum\": 0, \"pipelined\": false, \"replay\": 0, \"present_null\": %s, \"in_flight\": 1, "
               "\"input_format\": \"rgba\", \"output_format\": \"rgba\", \"protect_static\": %d, %s"
               "\"note\": \"nothing is presented: every second source frame is held out and compared on the GPU\", \"evaluation\": %s}\n",
               frames, (unsigned long long)result.pairs, result.seconds, presentNull ? "true" : "false", staticTolerance, filterField, result.json.c_str());
        return 0;
    }
    if (ranks > 0) {
        if (commFile.empty() || rank < 0 || rank >= ranks) { LOG_ERROR("--ranks needs --rank in range and --comm-file"); return 1; }
        if (!HipContext::Get().InitComm(ranks, rank, commFile, (uint64_t)commNonce)) { HipContext::Get().Cleanup(); return 1; }
        Scaler::Get().SetSharedPreviousSource(std::make_unique<SyntheticCapture>(0));   // the batch's previous frames: stream 0
        if (stream == 0) stream = (uint32_t)rank + 1;                                   // a rank's own current frames
    }
    {
        std::unique_ptr<FrameSource> source;
        if (!inputRaw.empty()) source = std::make_unique<RawFileCapture>(inputRaw, inputNv12);
        else source = std::make_unique<SyntheticCapture>(stream);
        if (replay > 0) source = std::make_unique<ReplayCapture>(std::move(source), (uint32_t)replay);
        Scaler::Get().SetFrameSource(std::move(source));
    }
    Scaler::Get().SetPipelined(!syncPresent);
    Scaler::Get().SetFramesInFlight(inFlight);
    Scaler::Get().SetCutCounting(cutThreshold >= 0);
    Scaler::Get().SetRealFrameFirst(generation == LFG_GENERATION_EXTRAPOLATE);
    Scaler::Get().SetNv12(inputNv12, outputNv12, yuv);
    if (!factors.empty()) Scaler::Get().SetInterpolationFactors(factors);
    FILE* rawOut = nullptr;
    if (!outputRaw.empty()) {
        rawOut = outputRaw == "-" ? stdout : fopen(outputRaw.c_str(), "wb");
        if (!rawOut) { LOG_ERROR("Cannot open ", outputRaw); return 1; }
    }
    FILE* report = rawOut == stdout ? stderr : stdout;          // keep the pixel stream clean
    uint64_t checksum = 0, presented = 0, generated = 0;
    Scaler::Get().SetPresenter([&](const uint8_t* rgba, uint32_t w, uint32_t h, bool interpolated) {
        const size_t n = Scaler::Get().PresentedBytes(w, h);    // (NV12 with --output-format nv12)
        uint64_t s = 0;
        if (!presentNull) for (size_t i = 0; i < n; i += 64) s += rgba[i];
        checksum = checksum * 1315423911ull + s;
        if (!dumpDir.empty()) {
            char name[512];
            snprintf(name, sizeof name, "%s/frame_%04llu_%s_%ux%u.%s", dumpDir.c_str(), (unsigned long long)presented,
                     interpolated ? "interp" : "real", w, h, outputNv12 ? "nv12" : "rgba");
            if (FILE* f = fopen(name, "wb")) { fwrite(rgba, 1, n, f); fclose(f); }
        }
        if (rawOut) fwrite(rgba, 1, n, rawOut);
        ++presented;
        generated += interpolated ? 1 : 0;
    });
    if (!Scaler::Get().Initialize(config)) {
        LOG_ERROR("Failed to initialize scaler");
        FrameManager::Get().Cleanup();
        HipContext::Get().Cleanup();
        return 1;
    }

    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    for (int i = 0; i < frames && ok; ++i) ok = Scaler::Get().ProcessFrame();
    ok = ok && Scaler::Get().Flush();                           // the last call's frames
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    const uint64_t cuts = Scaler::Get().GetCuts();
    // Teardown order as src/main.cpp:138-141.
    Scaler::Get().Cleanup();
    FrameManager::Get().Cleanup();
    HipContext::Get().Cleanup();
    if (!ok) { LOG_ERROR("ProcessFrame failed: ", Logger::Get().GetLastError()); return 1; }
    if (rawOut && rawOut != stdout) fclose(rawOut);
    char sharpenField[32] = "";
    if (config.sharpen > 0) snprintf(sharpenField, sizeof sharpenField, "\"sharpen\": %u, ", config.sharpen);
    char filterField[48] = "";
    if (config.scaleFilter >= 0) snprintf(filterField, sizeof filterField, "\"scale_filter\": \"%s\", ", kScaleFilterNames[config.scaleFilter]);
    char routeFields[120] = "";
    int used = 0;
    if (bidirectional >= 0) used = snprintf(routeFields, sizeof routeFields, "\"bidirectional\": %d, ", bidirectional);
    if (halfResMotion >= 0) used += snprintf(routeFields + used, sizeof routeFields - (size_t)used, "\"half_res_motion\": %d, ", halfResMotion);
    if (holeReach >= 1) used += snprintf(routeFields + used, sizeof routeFields - (size_t)used, "\"hole_reach\": %d, ", holeReach);
    if (config.subpelVectors >= 0) snprintf(routeFields + used, sizeof routeFields - (size_t)used, "\"subpel_vectors\": %d, ", config.subpelVectors);
    fprintf(report, "{\"input_frames\": %d, \"presented\": %llu, \"interpolated\": %llu, \"cuts\": %llu, \"seconds\": %.4f, "
           "\"presented_fps\": %.2f, \"checksum\": %llu, \"pipelined\": %s, \"replay\": %d, \"present_null\": %s, \"in_flight\": %d, "
           "\"input_format\": \"%s\", \"output_format\": \"%s\", \"protect_static\": %d, %s%s%s"
           "\"note\": \"includes %s, PCIe upload and readback\"}\n",
           frames, (unsigned long long)presented, (unsigned long long)generated, (unsigned long long)cuts, sec, presented / sec,
           (unsigned long long)checksum, syncPresent ? "false" : "true", replay, presentNull ? "true" : "false", inFlight,
           inputNv12 ? "nv12" : "rgba", outputNv12 ? "nv12" : "rgba", staticTolerance, sharpenField, filterField, routeFields,
           replay > 0 ? "one memcpy per input frame into the staging slot" : "host frame synthesis");
    return 0;
}
