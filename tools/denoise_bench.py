"""Measure lfg_denoise_temporal: what a call costs, what it gains, and what it does to the motion stage behind it.

  time     HIP events around every call, `--calls` calls after `--warmup` of warm-up: 1080p and 4K; radius 0, 1 and 2; one and two
           references; a pan (the vectors of lfg_motion on the device), a still (zero vectors) and uncorrelated frames (random
           vectors of up to 16 px).  In the same run, as yardsticks, lfg_motion_refine at the three radii on the same frames and
           fields, and lfg_sharpen at strength 16.  Every call works on the same buffers again, so they are served from the
           Infinity Cache: the quotients compare like with like, the times are no HBM figures.
  psnr     a 1080p pan by (3, -2) with +-2, +-4 and +-8 levels of noise, six frames filtered recursively on the vectors of
           lfg_motion(previous output, noisy frame): PSNR over R, G and B against the clean frame (lfg_frame_diff), of the last
           noisy frame and of the last output.
  motion   lfg_motion's time on (filtered previous frame, noisy frame) against (noisy previous frame, noisy frame), same stream.

    python tools/denoise_bench.py [--calls 100] [--warmup 10] [--sizes 1080p,4k] [--json out.json] [--out profile.txt]
"""
from __future__ import annotations

import hashlib
import json
import math
import sys

import numpy as np

from diff_bench import Events                                # (stage_bench, imported there, puts the repository root on sys.path)
from stage_bench import SIZES, emit, write_json
from linux_fg_amd import capi, synth  # noqa: E402
from tests import denoise_cases as dc  # noqa: E402

RADII = (0, 1, 2)
PARAMS = (32, 192, 255)                                      # tolerance, strength, limit


def time_contents(ctx, w, h):
    """(name, curr, [ref, ref2], [mv, mv2]) as device frames; fields on curr's grid."""
    mv_frame = lambda: ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    prev = synth.make_prev(w, h)
    curr = synth.translate(prev, synth.DEFAULT_SHIFT)
    nxt = synth.translate(curr, synth.DEFAULT_SHIFT, synth.BASE_SEED + 1)
    c, refs, mvs = ctx.frame_from(curr), [ctx.frame_from(prev), ctx.frame_from(nxt)], [mv_frame(), mv_frame()]
    for r, m in zip(refs, mvs):
        ctx.motion(r, c, m)
    ctx.sync()
    yield "pan", c, refs, mvs
    zero = np.zeros((h, w, 2), np.int8)
    yield "still", ctx.frame_from(prev), [ctx.frame_from(prev), ctx.frame_from(prev)], [ctx.frame_from(zero, capi.FORMAT_MV_S8X2) for _ in range(2)]
    rng = np.random.default_rng(3)
    frames = [ctx.frame_from(rng.integers(0, 256, (h, w, 4), dtype=np.uint8)) for _ in range(3)]
    fields = [ctx.frame_from(rng.integers(-16, 17, (h, w, 2), dtype=np.int8), capi.FORMAT_MV_S8X2) for _ in range(2)]
    yield "uncorrelated", frames[0], frames[1:], fields


def part_time(ctx, a, rows):
    events = Events(ctx, a.calls)
    for size in a.sizes.split(","):
        w, h = SIZES[size]
        out, mv_out = ctx.create_frame(w, h), ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
        for name, c, refs, mvs in time_contents(ctx, w, h):
            base = {"part": "time", "size": size, "content": name}
            med, mean = events.per_call_us(ctx, lambda: ctx.sharpen(c, out, 16), a.warmup)
            emit(rows, {**base, "call": "lfg_sharpen 16", "median_us": med, "mean_us": mean})
            refine = {}
            for radius in RADII:
                refine[radius], mean = events.per_call_us(ctx, lambda: ctx.motion_refine(refs[0], c, mvs[0], mv_out, radius), a.warmup)
                emit(rows, {**base, "call": "lfg_motion_refine", "radius": radius, "median_us": refine[radius], "mean_us": mean})
            for radius in RADII:
                for count in (1, 2):
                    med, mean = events.per_call_us(ctx, lambda: ctx.denoise_temporal(c, refs[:count], mvs[:count], out, radius, *PARAMS), a.warmup)
                    emit(rows, {**base, "call": "lfg_denoise_temporal", "radius": radius, "refs": count, "median_us": med, "mean_us": mean,
                                "of_refine_same_radius": med / refine[radius]})
            for f in [c] + refs + mvs:
                ctx.destroy_frame(f)
        ctx.destroy_frame(out)
        ctx.destroy_frame(mv_out)


def psnr(ctx, a, b, record, pixels):
    ctx.frame_diff(a, b, record, 0x7)
    sse = sum(ctx.read_diff_record(record)[1][:3])
    return 10.0 * math.log10(255.0 ** 2 * 3 * pixels / sse) if sse else float("inf")


def part_quality(ctx, a, rows):
    w, h = SIZES["1080p"]
    frames = 6
    events = Events(ctx, a.calls)
    clean = dc.pan_stream(w, h, frames, synth.DEFAULT_SHIFT)
    truth, record, mv = ctx.frame_from(clean[-1]), ctx.create_diff_record(), ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    pong = [ctx.create_frame(w, h), ctx.create_frame(w, h)]
    for amplitude in (2, 4, 8):
        noisy = [ctx.frame_from(dc.noisy(f, amplitude, 3000 + k)) for k, f in enumerate(clean)]
        prev = noisy[0]
        for k in range(1, frames):
            ctx.motion(prev, noisy[k], mv)
            ctx.denoise_temporal(noisy[k], [prev], [mv], pong[k % 2], 1, *PARAMS)
            before_last = prev                                  # the filtered frame k - 1 (the noisy frame 0 at k = 1)
            prev = pong[k % 2]
        emit(rows, {"part": "psnr", "size": "1080p", "noise": amplitude, "frames": frames, "radius": 1, "params": list(PARAMS),
                    "psnr_in_db": psnr(ctx, noisy[-1], truth, record, w * h), "psnr_out_db": psnr(ctx, prev, truth, record, w * h)})
        noisy_us, _ = events.per_call_us(ctx, lambda: ctx.motion(noisy[-2], noisy[-1], mv), a.warmup)
        filtered_us, _ = events.per_call_us(ctx, lambda: ctx.motion(before_last, noisy[-1], mv), a.warmup)
        emit(rows, {"part": "motion", "size": "1080p", "noise": amplitude, "noisy_prev_us": noisy_us, "filtered_prev_us": filtered_us,
                    "filtered_of_noisy": filtered_us / noisy_us})
        for f in noisy:
            ctx.destroy_frame(f)
    cleans = [ctx.frame_from(f) for f in clean[-2:]]
    clean_us, _ = events.per_call_us(ctx, lambda: ctx.motion(cleans[0], cleans[1], mv), a.warmup)
    emit(rows, {"part": "motion", "size": "1080p", "noise": 0, "clean_us": clean_us})


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--parts", default="time,psnr")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        if "time" in a.parts.split(","):
            part_time(ctx, a, rows)
        if "psnr" in a.parts.split(","):
            part_quality(ctx, a, rows)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/denoise_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; of_refine_same_radius = the call's median over lfg_motion_refine's at that radius on the\n"
                    "# same frames and field, in the same run.  Every call works on the same buffers again (Infinity Cache, no HBM figures).\n"
                    "# psnr: over R, G and B against the clean frame, by lfg_frame_diff; motion: lfg_motion's median under the intended\n"
                    "# semantics on the last pair of the stream, its previous frame noisy or filtered.\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
