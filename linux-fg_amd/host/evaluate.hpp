// lfg_host --evaluate: how close the generated frames come to frames that were held out.  No reference counterpart (its
// roadmap lists "Evaluate quality and performance metrics" as open).  Source frames 0, 2, 4, ... are the stream and 1, 3, 5, ...
// the truth; every frame is upscaled to the output size, where a viewer would look, and per pair k
//     lfg_interpolate_frames(up[2k], up[2k+2], out, 0.5)          under the context's settings, whatever they are
//     lfg_frame_diff(out,    up[2k+1], generated, 0xF, k > 0)
//     lfg_frame_diff(up[2k], up[2k+1], repeated,  0xF, k > 0)     the yardstick: showing the previous frame again
// on one lane, with no wait before the end: one lfg_sync, one download of both records, lfg_frame_diff_summarize on each.
// Beside each lfg_frame_diff an lfg_frame_ssim of the same two frames goes into a record of its own (downloaded with the
// others, summarized by lfg_frame_ssim_summarize into the object's "ssim" key), unless the output is smaller than one 8 x 8
// window in either dimension: then no such call is made and the key is null.
// Nothing is presented.  Scaler::ProcessFrame is not involved.
#pragma once
#include <string>

#include "frame_source.hpp"

struct EvaluationResult {
    uint64_t pairs = 0;
    double seconds = 0.0;
    std::string json;              // {"pairs": P, "generated": {...}, "repeated": {...}}
};

// `frames` >= 3 source frames of inputWidth x inputHeight from `source` (a trailing unpaired frame is not read), compared at
// outputWidth x outputHeight.  HipContext must be initialized and carry the settings to evaluate.
// With `extrapolate` (the context then carries LFG_GENERATION_EXTRAPOLATE) pair k's frames 2k and 2k + 1 give the frame one interval
// ahead, which "generated" compares with frame 2k + 2; "repeated" compares frame 2k + 1, the newest frame shown again, with it.
// The same frames are read and the report has the same keys.
// `scaleFilter` as ScalerConfig::scaleFilter: -1 upscales with lfg_scale, an lfg_filter with lfg_resample.
bool RunEvaluation(FrameSource& source, uint32_t inputWidth, uint32_t inputHeight, uint32_t outputWidth, uint32_t outputHeight,
                   int frames, EvaluationResult& result, bool extrapolate = false, int scaleFilter = -1);
