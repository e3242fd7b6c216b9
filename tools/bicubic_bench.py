"""Time and judge the bicubic fetch of the compensated routes.
  * lfg_interpolate_compensated_sampled at 1080p and 4K with LFG_SAMPLING_BICUBIC next to LFG_SAMPLING_BILINEAR on the same
    frames and field, on an even integer pan (every fetch on a texel: the single-texel path), an odd integer pan (half a pixel
    everywhere at t = 0.5), the refined fractional pan of tools/subpel_bench.py and uncorrelated frames under their refined field.
    The bilinear call is timed before and after the bicubic one; the distance between its two medians is the run's only margin.
  * quality with lfg_frame_diff on the held-out frames of subpel_bench's fractional stream and of its integer pan at 1080p:
    lfg_interpolate_frames under the pyramid and the compensated interpolator, bilinear against bicubic, with integer vectors
    and under lfg_set_subpixel_vectors 0, 1 and 2.
Device-event timing (lfg_profile_*: HIP events around the stage's launches -- the clear, the projection and the sampling kernel):
one sample per call, 200 calls after 20 of warm-up by default, medians.

    python tools/bicubic_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--json out.json] [--no-quality | --quality-only]
"""
from __future__ import annotations

import sys

import numpy as np

from stage_bench import SIZES, emit, write_json      # (puts the repository root on sys.path)
from subpel_bench import MV, MVQ, median_ms, pan_frames
from linux_fg_amd import capi  # noqa: E402

BILINEAR, BICUBIC = capi.SAMPLING_BILINEAR, capi.SAMPLING_BICUBIC


def contents(w, h):
    """(name, prev, curr, integer vectors, whether the field is refined to quarter pixels first)."""
    a, b = pan_frames(w, h, [(0, 0), (8, -8)])
    yield "even_integer_pan", a, b, (2, -2), False
    a, b = pan_frames(w, h, [(0, 0), (12, -4)])
    yield "odd_integer_pan", a, b, (3, -1), False
    a, b = pan_frames(w, h, [(0, 0), (10, -6)])
    yield "fractional_pan_refined", a, b, (3, -1), True
    rng = np.random.default_rng(11)
    yield "uncorrelated_refined", rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8), (0, 0), True


def timing(ctx, rows, size, calls, warmup):
    w, h = SIZES[size]
    for name, prev, curr, v, refined in contents(w, h):
        p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
        mv = np.zeros((h, w, 2), np.int8)
        mv[...] = v
        field = ctx.frame_from(mv, MV)
        if refined:
            q = ctx.create_frame(w, h, MVQ)
            ctx.motion_subpel(p, c, field, q, 1)
            ctx.sync()
            ctx.destroy_frame(field)
            field = q
        t = lambda sampling: round(median_ms(ctx, lambda: ctx.interpolate_compensated_sampled(p, c, field, o, 0.5, 48, sampling), calls, warmup,
                                             capi.STAGE_INTERPOLATE), 4)
        r = {"size": size, "content": name, "field": "q2" if refined else "s8"}
        r["bilinear_before_ms"], r["bicubic_ms"], r["bilinear_after_ms"] = t(BILINEAR), t(BICUBIC), t(BILINEAR)
        r["bilinear_spread_ms"] = round(abs(r["bilinear_after_ms"] - r["bilinear_before_ms"]), 4)
        r["quotient"] = round(r["bicubic_ms"] / (0.5 * (r["bilinear_before_ms"] + r["bilinear_after_ms"])), 3)
        emit(rows, r)
        for f in (p, c, o, field):
            ctx.destroy_frame(f)


def quality(ctx, rows, w, h):
    """Frames 0, 2, 4 are the stream and 1, 3 are held out (subpel_bench.quality's streams, 32 px cells)."""
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    ctx.set_motion_estimator(capi.ESTIMATOR_PYRAMID)
    ctx.set_interpolator(capi.INTERPOLATOR_COMPENSATED, 48)
    record, out = ctx.create_diff_record(), ctx.create_frame(w, h)
    for name, step in (("fractional_pan", (5, -3)), ("integer_pan", (4, -4))):
        frames = [ctx.frame_from(f) for f in pan_frames(w, h, [(k * step[0], k * step[1]) for k in range(5)], cell=32)]
        for radius in (-1, 0, 1, 2):
            ctx.set_subpixel_vectors(radius)
            r = {"quality": name, "size": f"{w}x{h}", "subpel_vectors": radius}
            for label, sampling in (("bilinear", BILINEAR), ("bicubic", BICUBIC)):
                ctx.set_sampling(sampling)
                assert ctx.sampling_effective() == sampling
                for k in (0, 2):
                    ctx.interpolate_frames(frames[k], frames[k + 2], out, 0.5)
                    ctx.frame_diff(out, frames[k + 1], record, 0xF, accumulate=k > 0)
                s = capi.summarize(ctx.read_diff_record(record))
                r[label + "_psnr_db"], r[label + "_differing"] = round(s["psnr_db"], 3), s["differing"]
            emit(rows, r)
        for f in frames:
            ctx.destroy_frame(f)
    ctx.set_sampling(BILINEAR)
    ctx.set_subpixel_vectors(-1)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        for size in [] if a.quality_only else a.sizes.split(","):
            timing(ctx, rows, size, a.calls, a.warmup)
        if not a.no_quality:
            quality(ctx, rows, 1920, 1080)
    write_json(a.json, rows)


if __name__ == "__main__":
    sys.exit(main())
