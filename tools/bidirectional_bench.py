"""Time lfg_interpolate_compensated_bidirectional beside lfg_interpolate_compensated on the same inputs in the same run, with one
factor and with three (t = 1/4, 1/2, 3/4), at 1080p and 4K on four contents of tools/compensated_bench.py: pan, moving block,
uncorrelated, dense random fields.  HIP events around every call, 200 calls after 20 of warm-up, medians; the vectors come from
lfg_motion run both ways under the intended semantics, except for the random fields, which are two independent draws.  The
compensated call is timed before and after the bidirectional one: the distance between its two medians is the run's own spread.
The motion stage that the switch doubles is no part of these figures (tools/stage_bench.py times it).

    python tools/bidirectional_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--tolerance 1] [--json out.json]
"""
from __future__ import annotations

import argparse

import numpy as np

import overlay_bench  # noqa: F401                            # (its imports put the repository root on sys.path)
from compensated_bench import FACTORS, contents
from diff_bench import Events
from stage_bench import SIZES, emit, write_json
from linux_fg_amd import capi  # noqa: E402

CONTENTS = ("pan(6,-4)", "square(12,0)", "uncorrelated", "random-mv,sad1020")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--tolerance", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        events = Events(ctx, a.calls)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr, vectors, ms in contents(w, h):
                if name not in CONTENTS:
                    continue
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                if vectors is None:
                    f, b = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2), ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                    ctx.motion(p, c, f)
                    ctx.motion(c, p, b)
                else:
                    f = ctx.frame_from(vectors, capi.FORMAT_MV_S8X2)
                    b = ctx.frame_from(np.random.default_rng(6).integers(-128, 128, (h, w, 2)).astype(np.int8), capi.FORMAT_MV_S8X2)
                outs = [ctx.create_frame(w, h) for _ in FACTORS]
                buf, mask = ctx.create_mask(w, h)

                def us(fn):
                    return round(events.per_call_us(ctx, fn, a.warmup)[0], 2)                                   # the median

                r = {"size": size, "content": name, "match_sad": ms, "tolerance": a.tolerance}
                compensated = lambda: ctx.interpolate_compensated(p, c, f, outs[0], 0.5, ms)  # noqa: E731
                r["compensated_us"] = us(compensated)
                r["bidirectional_us"] = us(lambda: ctx.interpolate_compensated_bidirectional(p, c, f, b, outs[0], 0.5, ms, a.tolerance))
                r["compensated_again_us"] = us(compensated)
                r["compensated_x3_us"] = us(lambda: ctx.interpolate_compensated_multi(p, c, f, outs, FACTORS, ms))
                r["bidirectional_x3_us"] = us(lambda: ctx.interpolate_compensated_bidirectional_multi(p, c, f, b, outs, FACTORS, ms, a.tolerance))
                r["consistency_us"] = us(lambda: ctx.motion_consistency(f, b, a.tolerance, mask))
                emit(rows, r)
                for x in [p, c, f, b, buf] + outs:
                    ctx.destroy_frame(x)
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
