"""Time lfg_motion_pyramid next to the full search (lfg_motion 8 / 16), and lfg_interpolate_frames under both estimators, at
1080p and 4K on five contents.  Device-event timing (lfg_profile_*: HIP events around every stage launch), after warm-up.

    python tools/pyramid_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--json out.json]
"""
from __future__ import annotations

import json

import numpy as np

from stage_bench import SIZES, arguments, emit, per_call_ms, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402

def contents(w, h):
    prev = synth.make_prev(w, h)
    rng = np.random.default_rng(1)
    noisy = np.clip(prev.astype(np.int16) + rng.integers(-4, 5, prev.shape), 0, 255).astype(np.uint8)
    yield "translated(3,-2)", prev, synth.translate(prev, (3, -2))
    yield "pan(40,-24)", prev, synth.translate(prev, (40, -24))
    a, b = synth.make_uncorrelated_pair(w, h)
    yield "uncorrelated", a, b
    yield "noise+-4", prev, noisy
    yield "static", prev, prev.copy()


def per_call(ctx, fn, calls, warmup):
    return per_call_ms(ctx, fn, calls, warmup, capi.STAGE_MOTION, capi.STAGE_INTERPOLATE)


def main():
    a = arguments("1080p,4k")
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                o = ctx.create_frame(w, h)
                r = {"size": size, "content": name}
                r["pyramid_ms"] = per_call(ctx, lambda: ctx.motion_pyramid(p, c, m, 2, 16, 2), a.calls, a.warmup)
                r["full_search_ms"] = per_call(ctx, lambda: ctx.motion(p, c, m), a.calls, a.warmup)
                for est, key in ((capi.ESTIMATOR_PYRAMID, "frames_pyramid_ms"), (capi.ESTIMATOR_FULL_SEARCH, "frames_full_ms")):
                    ctx.set_motion_estimator(est)
                    r[key] = per_call(ctx, lambda: ctx.interpolate_frames(p, c, o, 0.5), a.calls, a.warmup)
                ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
                emit(rows, r)
                for f in (p, c, m, o):
                    ctx.destroy_frame(f)
    for size in a.sizes.split(","):
        t = [r["pyramid_ms"] for r in rows if r["size"] == size]
        print(json.dumps({"size": size, "pyramid_min_ms": min(t), "pyramid_max_ms": max(t),
                          "pyramid_spread_pct": 100.0 * (max(t) - min(t)) / min(t)}))
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
