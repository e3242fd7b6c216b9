"""Time the scene-cut detection: lfg_pair_match alone at 1080p, 4K and 8K on a pan (lfg_motion's vectors under the intended
semantics), on uncorrelated frames (lfg_motion's) and on dense random vectors; lfg_cut_fallback at 4K without a cut and with
one; and lfg_interpolate_frames at 4K with detection off and at 500, for full search + shader and for pyramid + compensated,
on the pan and on a cut.  Device-event timing (lfg_profile_*: HIP events around every stage launch), 200 calls after 20 of
warm-up by default.

    python tools/cut_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--yardstick]

--yardstick also runs lfg_interpolate_compensated(t = 0.5) on every input of the first part, so that a kernel trace of the
run (rocprofv3 --kernel-trace --stats -- python tools/cut_bench.py --yardstick ...) holds mc_project_kernel, which makes the
same loads plus one atomic per pixel, next to pair_match_kernel on the same inputs, in the same order.
"""
from __future__ import annotations

import sys

import numpy as np

from stage_bench import SIZES, arguments, emit, per_call_ms, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402

THRESHOLD = 500


def contents(w, h):
    """(name, prev, curr, vectors or the estimator that makes them)"""
    prev = synth.make_prev(w, h)
    yield "pan(6,-4)", prev, synth.translate(prev, (6, -4)), "full"
    a, b = synth.make_uncorrelated_pair(w, h)
    yield "uncorrelated", a, b, "full"
    yield "random-mv", a, b, np.random.default_rng(5).integers(-128, 128, (h, w, 2)).astype(np.int8)


def pair_match_rows(ctx, a, rows, yardstick):
    for size in a.sizes.split(","):
        w, h = SIZES[size]
        for name, prev, curr, vectors in contents(w, h):
            p, c = ctx.frame_from(prev), ctx.frame_from(curr)
            if isinstance(vectors, str):
                m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                ctx.motion(p, c, m)
            else:
                m = ctx.frame_from(vectors, capi.FORMAT_MV_S8X2)
            r = ctx.create_pair_record()
            us = 1000.0 * per_call_ms(ctx, lambda: ctx.pair_match(p, c, m, r, 48), a.calls, a.warmup, capi.STAGE_MOTION)
            pixels, matched, sad_sum = ctx.read_pair_record(r)
            row = {"part": "pair_match", "size": size, "content": name, "matched_permille": matched * 1000 // pixels,
                   "pair_match_us": us, "gbytes_per_s": 10.0 * pixels / us / 1000.0}
            if yardstick:
                o = ctx.create_frame(w, h)
                row["compensated_us"] = 1000.0 * per_call_ms(ctx, lambda: ctx.interpolate_compensated(p, c, m, o, 0.5, 48),
                                                            a.calls, a.warmup, capi.STAGE_INTERPOLATE)
                ctx.destroy_frame(o)
            emit(rows, row)
            for f in (p, c, m, r):
                ctx.destroy_frame(f)


def fallback_rows(ctx, a, rows):
    w, h = SIZES["4k"]
    prev = synth.make_prev(w, h)
    p, c, o = ctx.frame_from(prev), ctx.frame_from(synth.translate(prev, (6, -4))), ctx.create_frame(w, h)
    r = ctx.create_pair_record()
    for name, matched in (("no cut", w * h), ("cut", 0)):
        ctx.write_pair_record(r, w * h, matched, 0)
        us = 1000.0 * per_call_ms(ctx, lambda: ctx.cut_fallback(p, c, r, THRESHOLD, [o], [0.5]), a.calls, a.warmup, capi.STAGE_INTERPOLATE)
        emit(rows, {"part": "cut_fallback", "size": "4k", "content": name, "cut_fallback_us": us})
    for f in (p, c, o, r):
        ctx.destroy_frame(f)


def frames_rows(ctx, a, rows):
    w, h = SIZES["4k"]
    prev = synth.make_prev(w, h)
    pairs = [("pan(6,-4)", prev, synth.translate(prev, (6, -4))), ("cut", prev, synth.make_prev(w, h, synth.BASE_SEED + 1))]
    routes = [("full+shader", capi.ESTIMATOR_FULL_SEARCH, capi.INTERPOLATOR_SHADER),
              ("pyramid+compensated", capi.ESTIMATOR_PYRAMID, capi.INTERPOLATOR_COMPENSATED)]
    for name, x, y in pairs:
        p, c, o = ctx.frame_from(x), ctx.frame_from(y), ctx.create_frame(w, h)
        for route, estimator, interpolator in routes:
            ctx.set_motion_estimator(estimator)
            ctx.set_interpolator(interpolator)
            row = {"part": "interpolate_frames", "size": "4k", "content": name, "route": route}
            for label, threshold in (("off", -1), ("at_500", THRESHOLD)):
                ctx.set_cut_detection(threshold)
                row[f"{label}_us"] = 1000.0 * per_call_ms(ctx, lambda: ctx.interpolate_frames(p, c, o, 0.5), a.calls, a.warmup,
                                                          capi.STAGE_MOTION, capi.STAGE_INTERPOLATE)
                if threshold >= 0:
                    (pixels, matched, _), cut = ctx.last_pair_stats()
                    row["matched_permille"], row["cut"] = matched * 1000 // pixels, cut
            ctx.set_cut_detection(-1)
            emit(rows, row)
        for f in (p, c, o):
            ctx.destroy_frame(f)
    ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
    ctx.set_interpolator(capi.INTERPOLATOR_SHADER)


def main():
    yardstick = "--yardstick" in sys.argv
    if yardstick:
        sys.argv.remove("--yardstick")
    a = arguments("1080p,4k,8k")
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        pair_match_rows(ctx, a, rows, yardstick)
        fallback_rows(ctx, a, rows)
        frames_rows(ctx, a, rows)
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
