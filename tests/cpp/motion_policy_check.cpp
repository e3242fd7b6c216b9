// Test helper (CPU only): holds the motion launch policy of csrc/lfg_motion_verdict.hpp to the expressions motion_run
// (csrc/lfg_capi.cpp) used before the policy moved there, copied below verbatim, over the whole input space that matters.
// Prints "ok <cases>" and exits 0, or prints the first difference and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lfg_motion_verdict.hpp"

namespace {

// The pre-refactor state: the selected lane's fields as they sat on the context.
struct OldContext {
    std::vector<int> lanes;
    bool motion_hints = true;
    struct { int rimSplit2 = 0, leanCount = 0, lastLean = 0; } motion_ws_layout;
    uint32_t *lean_flag = nullptr;
    bool lean_ev_pending = false;
    int lean_predict = 0;
    bool lean_seen = false;
    uint32_t lean_request_guess = 0;
    int motion_slots = 0, device_cus = 0, comm_cus = 0;
    lfg::MotionKnobs knobs;
    uint64_t pred_verdicts = 0, pred_lean_wrong = 0, pred_grid_wrong = 0, pred_second_wrong = 0;
};

int persistent_grid_most(const OldContext *ctx) {
    if (ctx->comm_cus <= 0 || ctx->device_cus <= ctx->comm_cus) return ctx->motion_slots;
    return ctx->motion_slots / ctx->device_cus * (ctx->device_cus - ctx->comm_cus);
}

struct OldCall {
    int lastLean, groupsCap, tier;
    bool expectNoFallback;
    uint32_t *hostWord;
    bool recorded;
    uint32_t guess;
};

// motion_run's decisions, verbatim but for lean_frames_ok (a flag here) and the HIP calls (left out).
OldCall old_policy(OldContext *ctx, bool fused, bool framesOk, bool othersBusy) {
    struct { void *data; } fo{fused ? (void *)ctx : nullptr};
    const bool leanPossible = ctx->motion_ws_layout.rimSplit2 != 0 && ctx->motion_hints;
    const bool flagWanted = ctx->lanes.size() >= 2 && ctx->motion_hints;
    if (ctx->knobs.leanForce >= 0) ctx->lean_predict = (ctx->lean_predict & ~1) | ctx->knobs.leanForce;          // (measurement: 1 = every call, 0 = none)
    ctx->motion_ws_layout.lastLean = (leanPossible && ctx->motion_ws_layout.leanCount > 0 && (ctx->lean_predict & 1) != 0 && !fo.data && framesOk) ? 1 : 0;
    int groupsCap = (flagWanted && othersBusy && ((uint32_t)ctx->lean_predict >> 31) != 0u) ? std::max(1, ctx->motion_slots * 5 / 8) : 0;
    if (ctx->comm_cus > 0) groupsCap = groupsCap ? std::min(groupsCap, persistent_grid_most(ctx)) : persistent_grid_most(ctx);
    const int tier = ctx->knobs.tierForce >= 0 ? ctx->knobs.tierForce : (flagWanted && ctx->lean_seen && (((uint32_t)ctx->lean_predict >> 29) & 1u)) ? 1 : 0;
    const bool expectNoFallback = flagWanted && ctx->lean_seen && (((uint32_t)ctx->lean_predict >> 30) & 1u) == 0u && !ctx->knobs.fallbackFull /* (measurement) */;
    OldCall c{ctx->motion_ws_layout.lastLean, groupsCap, tier, expectNoFallback, (flagWanted && !ctx->lean_ev_pending) ? ctx->lean_flag : nullptr, false, 0};
    if (flagWanted && !ctx->lean_ev_pending && !fo.data) {
        c.recorded = true;
        ctx->lean_request_guess = (ctx->motion_ws_layout.lastLean ? 1u : 0u) | ((leanPossible && ctx->motion_ws_layout.leanCount > 0) ? 2u : 0u) |
                                  ((uint32_t)ctx->lean_predict & 0x80000000u) | (expectNoFallback ? 1u << 30 : 0u) | (tier ? 1u << 29 : 0u);
        c.guess = ctx->lean_request_guess;
    }
    return c;
}

// The scoring of an arrived word, verbatim.
void old_score(OldContext *ctx, uint32_t word) {
    ctx->lean_predict = (int)word;
    const uint32_t said = (uint32_t)ctx->lean_predict, guess = ctx->lean_request_guess;
    ctx->pred_verdicts += 1;
    if ((guess & 2u) && ((guess ^ said) & 1u)) ctx->pred_lean_wrong += 1;
    if (((guess ^ said) >> 31) || (((guess ^ said) >> 29) & 1u)) ctx->pred_grid_wrong += 1;      // (the persistent launch: its grid, or its variant)
    if (((guess >> 30) & 1u) && ((said >> 30) & 1u)) ctx->pred_second_wrong += 1;       // (small grid, and tiles were flagged: the costly direction)
}

// A MotionLaunch in the old guess word's layout, and back.
uint32_t pack(const lfg::MotionLaunch &on) {
    return (on.lean ? 1u : 0u) | (on.leanAvailable ? 2u : 0u) | (on.mostMatchGrid ? 1u << 31 : 0u) | (on.smallSecondPass ? 1u << 30 : 0u) |
           (on.tier ? 1u << 29 : 0u);
}
lfg::MotionLaunch unpack(uint32_t guess) {
    lfg::MotionLaunch on;
    on.lean = guess & 1u; on.leanAvailable = (guess >> 1) & 1u; on.mostMatchGrid = guess >> 31; on.smallSecondPass = (guess >> 30) & 1u;
    on.tier = (int)((guess >> 29) & 1u);
    return on;
}

}  // namespace

int main() {
    // the verdict words: every combination of the bits the host reads, with and without counts below them
    std::vector<uint32_t> words;
    for (uint32_t b = 0; b < 16; ++b)
        for (uint32_t counts : {0u, (200u << 1) | (37u << 12)})
            words.push_back((b & 1u) | ((b >> 1) << 29) | counts);
    // the encoder against the layout the order kernel wrote by hand (motion_order.hip before the header)
    for (uint32_t close : {0u, 1u, 239u, 240u, 255u, 256u})
        for (uint32_t exact : {0u, 5u, 256u})
            for (uint32_t moderate : {0u, 127u, 128u, 256u})
                for (uint32_t most : {0u, 1u}) {
                    const uint32_t closeAll = close | (exact << 16), kHints = 256u;
                    const uint32_t want = (((closeAll & 0xFFFFu) * 16u >= 15u * (uint32_t)kHints) ? 1u : 0u) | ((closeAll & 0xFFFFu) << 1) |
                                          (((closeAll >> 16) & 0x7FFu) << 12) | ((moderate * 2u >= (uint32_t)kHints ? 1u : 0u) << 29) | (most << 31);
                    const uint32_t got = lfg::verdict_encode(closeAll, closeAll >> 16, moderate, kHints, most);
                    if (got != want || lfg::verdict_close(got) != close || lfg::verdict_exact(got) != exact ||
                        lfg::verdict_with_flagged(got, true) != (want | (1u << 30)) || lfg::verdict_with_flagged(got, false) != want) {
                        printf("encode differs: close %u exact %u moderate %u most %u: %#x against %#x\n", close, exact, moderate, most, got, want);
                        return 1;
                    }
                }
    uint64_t cases = 0;
    for (uint32_t word : words)
    for (int seen = 0; seen < 2; ++seen)
    for (int pending = 0; pending < 2; ++pending)
    for (int lanes = 1; lanes <= 3; ++lanes)
    for (int bools = 0; bools < 64; ++bools)
    for (int leanForce = -1; leanForce <= 1; ++leanForce)
    for (int tierForce = -1; tierForce <= 1; ++tierForce)
    for (int fallbackFull = 0; fallbackFull < 2; ++fallbackFull)
    for (int comm = 0; comm < 4; ++comm)
    for (int slots : {0, 1, 7, 1024, 2048}) {
        const bool hints = bools & 1, rimSplit2 = bools & 2, leanTiles = bools & 4, fused = bools & 8, framesOk = bools & 16, othersBusy = bools & 32;
        const int commCus = (comm & 1) ? 8 : 0, deviceCus = (comm & 2) ? 8 : 256;
        lfg::MotionKnobs knobs;
        knobs.leanForce = leanForce; knobs.tierForce = tierForce; knobs.fallbackFull = fallbackFull;

        uint32_t pinned = 0;
        OldContext old;
        old.lanes.assign((size_t)lanes, 0);
        old.motion_hints = hints;
        old.motion_ws_layout.rimSplit2 = rimSplit2 ? 48 : 0;
        old.motion_ws_layout.leanCount = leanTiles ? 1200 : 0;
        old.lean_flag = &pinned;
        old.lean_ev_pending = pending;
        old.lean_predict = (int)word;
        old.lean_seen = seen;
        old.motion_slots = slots; old.device_cus = deviceCus; old.comm_cus = commCus;
        old.knobs = knobs;
        const OldCall want = old_policy(&old, fused, framesOk, othersBusy);

        lfg::MotionVerdictState v;
        v.pinned = &pinned; v.pending = pending; v.word = word; v.seen = seen;
        lfg::MotionCallInputs in;
        in.lanes = lanes; in.hints = hints; in.leanPlan = rimSplit2 && leanTiles; in.fused = fused; in.leanFramesOk = framesOk;
        in.othersBusy = othersBusy; in.slots = slots; in.deviceCus = deviceCus; in.commCus = commCus;
        const lfg::MotionCall got = lfg::motion_call_policy(v, in, knobs);

        const bool same = (got.lean ? 1 : 0) == want.lastLean && got.groupsCap == want.groupsCap && got.tier == want.tier &&
                          got.expectNoFallback == want.expectNoFallback && (got.deliverWord ? &pinned : nullptr) == want.hostWord &&
                          got.awaitVerdict == want.recorded && (!want.recorded || pack(got.launchedOn) == want.guess) &&
                          lfg::motion_verdict_wanted(lanes, hints) == (lanes >= 2 && hints);
        if (!same) {
            printf("policy differs: word %#x seen %d pending %d lanes %d bools %#x leanForce %d tierForce %d fallbackFull %d commCus %d deviceCus %d slots %d\n"
                   "  old: lean %d cap %d tier %d small %d word %d record %d guess %#x\n  new: lean %d cap %d tier %d small %d word %d record %d guess %#x\n",
                   word, seen, pending, lanes, bools, leanForce, tierForce, fallbackFull, commCus, deviceCus, slots,
                   want.lastLean, want.groupsCap, want.tier, want.expectNoFallback, want.hostWord != nullptr, want.recorded, want.guess,
                   got.lean, got.groupsCap, got.tier, got.expectNoFallback, got.deliverWord, got.awaitVerdict, pack(got.launchedOn));
            return 1;
        }
        ++cases;
    }
    // the scoring: every guess the old word could carry against every verdict
    for (uint32_t g = 0; g < 32; ++g) {
        const uint32_t guess = (g & 3u) | ((g >> 2) << 29);
        for (uint32_t said : words) {
            OldContext old;
            old.lean_request_guess = guess;
            old_score(&old, said);
            const lfg::MotionVerdictScore s = lfg::motion_verdict_score(unpack(guess), said);
            if (pack(unpack(guess)) != guess || old.pred_verdicts != 1 || old.pred_lean_wrong != (uint64_t)s.leanWrong ||
                old.pred_grid_wrong != (uint64_t)s.gridWrong || old.pred_second_wrong != (uint64_t)s.secondWrong) {
                printf("score differs: guess %#x said %#x: old %d %d %d, new %d %d %d\n", guess, said, (int)old.pred_lean_wrong,
                       (int)old.pred_grid_wrong, (int)old.pred_second_wrong, s.leanWrong, s.gridWrong, s.secondWrong);
                return 1;
            }
            ++cases;
        }
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
