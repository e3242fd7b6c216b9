// What lfg_host's command line says: one Options struct, the table of option rows that fills it, the rules for what cannot be
// combined, and the report line.  Takes only constants from include/linuxfg_hip.h and calls nothing in the library, so
// options.cpp compiles and links with g++ alone (tests/cpp/host_options_check.cpp).  A new option is one row of kOptionRows, one
// field here and, for a library setting, one line of HipContext::SetRoute.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "scaler.hpp"

struct Options {
    ScalerConfig config;
    Route route;
    bool inputNv12 = false, outputNv12 = false;
    Scaler::YuvModes yuv;
    std::vector<float> factors;
    int inFlight = 2, ranks = 0, rank = 0;
    std::string commFile;
    unsigned long long commNonce = 0;                 // ParseOptions starts from LFG_COMM_NONCE
    int frames = 10, device = 0, replay = 0;
    uint32_t stream = 0;
    std::string dumpDir, inputRaw, outputRaw;
    bool help = false, quiet = false, evaluate = false, syncPresent = false, presentNull = false;
};

struct OptionRow {
    // Flag: no value.  Lenient: atoi of the value, whatever it is.  Whole: a whole number in [lo, hi], nothing before or after
    // it.  Name: one of the names in `bracket`, set() receives its index.  Text: set() reads the value itself.
    enum Kind { Flag, Lenient, Whole, Name, Text } kind;
    const char* name;
    long lo, hi;
    const char* bracket;                              // "Invalid NAME (BRACKET)": Whole's hint, Name's names with | between them
    bool (*set)(Options&, long, const char*);         // Text may return false: "Invalid NAME BRACKET"
};
extern const OptionRow kOptionRows[];
extern const size_t kOptionRowCount;
extern const char kUsage[];

// Both return the message of what they refuse, "" if nothing.  ParseOptions stops at --help (Options::help); an option that
// needs a value and stands last is read as the stream index, like every word that is no option.
std::string ParseOptions(int argc, const char* const* argv, Options& options);
// `tapsFit(filter, in, out)`: whether an lfg_filter scales one axis of `in` samples to `out` within LFG_RESAMPLE_MAX_TAPS.
std::string CheckOptions(const Options& options, const std::function<bool(int, uint32_t, uint32_t)>& tapsFit);

struct ReportCounters {                               // --evaluate: generated is the number of pairs, evaluation its JSON object
    uint64_t presented = 0, generated = 0, cuts = 0, checksum = 0;
    double seconds = 0.0;
    std::string evaluation;
};
std::string ReportLine(const Options& options, const ReportCounters& counters);
