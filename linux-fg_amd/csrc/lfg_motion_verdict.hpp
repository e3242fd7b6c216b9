// The verdict word of a motion call and the launch policy the host derives from it.  Host and device code share this header;
// it needs nothing but the standard library, so that tests/cpp/motion_policy_check.cpp can hold the policy to its
// pre-refactor form with g++ alone.
//
// The order kernel (motion_order.hip) judges each call's content from its sample blocks and writes one word, order32[kCand + 2]
// of the call's own order table; the second pass (motion_literal.hip) adds whether a tile was flagged and hands the word to the
// host through a pinned word.  The host learns it one call late and launches the lane's NEXT call by it (lfg_capi.cpp: motion_run).
#pragma once

#include <algorithm>
#include <cstdint>

struct ihipEvent_t;     // (hipEvent_t is a pointer to it)

namespace lfg {

// Bits and fields of the verdict word.
constexpr uint32_t kVerdictLean = 1u << 0;           // nearly every sample block matches closely: the lean kernel pays
constexpr int kVerdictCloseShift = 1;                // sample blocks with a close match (for LFG_DEBUG)
constexpr int kVerdictExactShift = 12;               // ... with an exact one (for LFG_DEBUG)
constexpr uint32_t kVerdictCountMask = 0x7FFu;
constexpr uint32_t kVerdictModerate = 1u << 29;      // half the sample blocks or more match moderately well: the persistent kernel's variant
constexpr uint32_t kVerdictFlagged = 1u << 30;       // the second pass found a tile flagged (the literal kernel ran)
constexpr uint32_t kVerdictMostMatch = 1u << 31;     // most sample blocks have a match at all

// The order kernel's word, from its counts over `samples` sample blocks: those with a close match (the lean kernel's reach; the
// field is written 16 bits wide, the count fits in 11), with an exact one, with a moderate one, and whether most of them match
// at all (0 | 1).  The bars: the lean kernel where 15 in 16 match closely, the variant where half of them match moderately well
// (motion_order.hip: motion_order_kernel says why).
constexpr uint32_t verdict_encode(uint32_t close, uint32_t exact, uint32_t moderate, uint32_t samples, uint32_t mostMatch) {
    return (((close & 0xFFFFu) * 16u >= 15u * samples) ? kVerdictLean : 0u) | ((close & 0xFFFFu) << kVerdictCloseShift) |
           ((exact & kVerdictCountMask) << kVerdictExactShift) | (moderate * 2u >= samples ? kVerdictModerate : 0u) |
           (mostMatch != 0u ? kVerdictMostMatch : 0u);
}
// ... and the second pass's addition to it.
constexpr uint32_t verdict_with_flagged(uint32_t word, bool flagged) { return word | (flagged ? kVerdictFlagged : 0u); }

constexpr bool verdict_lean(uint32_t word) { return (word & kVerdictLean) != 0u; }
constexpr uint32_t verdict_close(uint32_t word) { return (word >> kVerdictCloseShift) & kVerdictCountMask; }
constexpr uint32_t verdict_exact(uint32_t word) { return (word >> kVerdictExactShift) & kVerdictCountMask; }
constexpr bool verdict_moderate(uint32_t word) { return (word & kVerdictModerate) != 0u; }
constexpr bool verdict_flagged(uint32_t word) { return (word & kVerdictFlagged) != 0u; }
constexpr bool verdict_most_match(uint32_t word) { return (word & kVerdictMostMatch) != 0u; }

// Measurement knobs, read ONCE from the environment when a context is created (lfg_context_create) and never again: a call's
// launch geometry cannot change between two lfg_motion calls because somebody called setenv.  All of them are for A/B runs of
// tools/; none changes a result.
struct MotionKnobs {
    int leanForce = -1;       // LFG_LEAN_FORCE = 1: every call through the lean kernel whatever the verdict, 0: none, unset: by the verdict
    int fallbackFull = 0;     // LFG_FALLBACK_FULL: the second pass always on its full grid
    int dynParts = 0;         // LFG_DYN_PARTS_RT = 4 | 8: parts of a handed-over segment, whatever the lane count
    int prefGroups = 0;       // LFG_PREF_GROUPS: workgroups of the persistent kernel
    int resolveGroups = 0;    // LFG_RESOLVE_GROUPS: workgroups of the resolve kernel
    int strips = 0;           // LFG_MOTION_STRIP = 1: the exposed strips through a kernel of their own (motion_strip.hip: exact, measured slower)
    int stripPad = -1;        // LFG_STRIP_PAD: bytes of dynamic LDS a strip workgroup asks for on top of its own (-1: the launcher's choice)
    int debug = 0;            // LFG_DEBUG: reporting calls print what they read
    int debugDyn = 0;         // LFG_DEBUG_DYN: lfg_motion_last_stats prints the deepest private lists of the handed-over segments,
    int debugDynDeep = 14;    // LFG_DEBUG_DYN_DEEP: ... deeper than this
    int tierForce = -1;       // LFG_TIER_FORCE = 0 | 1: the persistent kernel's variant whatever the verdict (-1: by the verdict)
    int fillBand = 0;         // LFG_FILL_BAND = 8 .. 1024: rows per workgroup of lfg_hole_fill_plane's column pass (0: kFillBand; tools/fill_bench.py's band sweep)
    int commCus = 8;          // LFG_COMM_CUS = 0 | 8 | 16 | 24 | 32: CUs a communicator keeps free of the library's own kernels (lfg_comm.cpp)
};

// What a call was launched on -- held against the verdict its own content returns (lfg_motion_prediction_stats).
struct MotionLaunch {
    bool lean = false;                // it went through the lean kernel
    bool leanAvailable = false;       // ... which was available to it
    bool mostMatchGrid = false;       // its persistent grid was sized for "most sample blocks match"
    bool smallSecondPass = false;     // its second pass was the small looping grid
    int tier = 0;                     // the persistent kernel's variant
};

// A lane's verdicts: the pinned word the last launch that asked for one writes, the event behind that launch, and the word the
// lane's next call goes by.
struct MotionVerdictState {
    uint32_t *pinned = nullptr;
    ihipEvent_t *event = nullptr;     // hipEvent_t
    bool pending = false;             // a word is on its way
    uint32_t word = 0;                // the last word that arrived
    bool seen = false;                // ... and whether any has
    MotionLaunch launchedOn;          // what the call that carries the pending word was launched on
};

// Whether a lane's calls ask for verdicts at all: with frames in flight, and hints to judge by.
constexpr bool motion_verdict_wanted(int lanes, bool hints) { return lanes >= 2 && hints; }

// Workgroups of the persistent kernel a launch may have: what the device holds at once (slots) -- less the CUs a communicator
// keeps, where the library's streams cannot place any (lfg_own_stream_create).
constexpr int persistent_grid_most(int slots, int deviceCus, int commCus) {
    return (commCus <= 0 || deviceCus <= commCus) ? slots : slots / deviceCus * (deviceCus - commCus);
}

// What a call's launch depends on besides the lane's verdicts and the knobs.
struct MotionCallInputs {
    int lanes = 1;                    // the context's lane count
    bool hints = true;                // per-call visiting order (the order kernel: no verdict without it)
    bool leanPlan = false;            // the workspace holds the lean kernel's plan and tiles
    bool fused = false;               // the motion kernels write the generated frame (lfg_interpolate_frames)
    bool leanFramesOk = false;        // lean_frames_ok(prev, curr, mv)
    bool othersBusy = false;          // another lane has work queued or running
    int slots = 0;                    // persistent workgroups the device holds at once
    int deviceCus = 0, commCus = 0;   // the device's CUs, and those a communicator keeps
};

// What the call does.
struct MotionCall {
    bool lean = false;                // through the lean kernel first
    int groupsCap = 0;                // persistent workgroups at most (0: as many as the device holds)
    int tier = 0;                     // the persistent kernel's variant
    bool expectNoFallback = false;    // the second pass on its small looping grid
    bool deliverWord = false;         // the launch writes its verdict into the lane's pinned word
    bool awaitVerdict = false;        // ... and the host records the event behind it and waits for that word
    MotionLaunch launchedOn;          // what to score the word against (awaitVerdict)
};

inline MotionCall motion_call_policy(const MotionVerdictState &v, const MotionCallInputs &in, const MotionKnobs &knobs) {
    const bool wanted = motion_verdict_wanted(in.lanes, in.hints);
    const bool leanAvailable = in.leanPlan && in.hints;
    uint32_t word = v.word;
    if (knobs.leanForce >= 0) word = (word & ~kVerdictLean) | (uint32_t)knobs.leanForce;       // (measurement: 1 = every call, 0 = none)
    MotionCall c;
    // The lean kernel (motion_lean.hip) for content that suits it -- a pan, an object's motion: most sample blocks match nearly but
    // not exactly.  A kernel that finds out on the device that it has nothing to do still has to be placed, 2,144 workgroups of
    // 48 KB of LDS behind the other lanes' persistent kernels: -7 % on noisy frames, measured.
    c.lean = leanAvailable && verdict_lean(word) && !in.fused && in.leanFramesOk;
    // Where most sample blocks had a match the persistent kernel runs with 5/8 of the workgroups the device holds -- while another
    // lane has work: each draws more units, fewer slots idle in a launch's tail, and the other lanes' kernels find room beside it --
    // pan 3,660 -> 3,800 frames/s, stills +8 %, noise +3.7 %, occlusions and moving objects +2 %; frames without a match anywhere
    // (every segment searched in full: the slots are what they need) keep the full grid (5/8 there: -3.4 %).  A call that has the
    // device to itself takes the full grid, and is as long as on a context without lanes.
    c.groupsCap = (wanted && in.othersBusy && verdict_most_match(word)) ? std::max(1, in.slots * 5 / 8) : 0;
    if (in.commCus > 0) {
        const int most = persistent_grid_most(in.slots, in.deviceCus, in.commCus);
        c.groupsCap = c.groupsCap ? std::min(c.groupsCap, most) : most;
    }
    // The variant with the eight-point walk by SADs where half the sample blocks matched moderately well (sensor noise of +-3 .. +-6
    // levels at the input; motion_prefilter.hip, kTier).
    c.tier = knobs.tierForce >= 0 ? knobs.tierForce : (wanted && v.seen && verdict_moderate(word)) ? 1 : 0;
    // No tile went through the literal kernel last time (flat content under a fade, exact ties are what flags one): this call's
    // second pass is 64 workgroups instead of 2,048 -- they take whatever it flags after all, in turns (1.4 % of the frame rate
    // under a pan: workgroups of 42 KB of LDS that read a count and leave still have to be placed).
    c.expectNoFallback = wanted && v.seen && !verdict_flagged(word) && !knobs.fallbackFull;
    c.deliverWord = wanted && !v.pending;
    c.awaitVerdict = c.deliverWord && !in.fused;
    c.launchedOn.lean = c.lean;
    c.launchedOn.leanAvailable = leanAvailable;
    c.launchedOn.mostMatchGrid = verdict_most_match(word);
    c.launchedOn.smallSecondPass = c.expectNoFallback;
    c.launchedOn.tier = c.tier;
    return c;
}

// A returned verdict against what its call was launched on: the guesses the call's own content contradicted.
struct MotionVerdictScore {
    bool leanWrong = false;           // the lean kernel was available, and taken where the content did not suit it or the reverse
    bool gridWrong = false;           // the persistent launch: its grid, or its variant
    bool secondWrong = false;         // a small second pass where tiles were flagged (the costly direction)
};

constexpr MotionVerdictScore motion_verdict_score(const MotionLaunch &on, uint32_t said) {
    return MotionVerdictScore{on.leanAvailable && on.lean != verdict_lean(said),
                              on.mostMatchGrid != verdict_most_match(said) || (on.tier != 0) != verdict_moderate(said),
                              on.smallSecondPass && verdict_flagged(said)};
}

}  // namespace lfg
