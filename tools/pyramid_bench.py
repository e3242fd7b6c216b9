"""Time lfg_motion_pyramid next to the full search (lfg_motion 8 / 16), and lfg_interpolate_frames under both estimators, at
1080p and 4K on five contents.  Device-event timing (lfg_profile_*: HIP events around every stage launch), after warm-up.

    python tools/pyramid_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linux_fg_amd import capi, synth  # noqa: E402

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}


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


def per_call_ms(ctx, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(calls):
        fn()
    ms = [ctx.profile_get(s)[0] for s in (capi.STAGE_MOTION, capi.STAGE_INTERPOLATE)]
    ctx.profile_enable(False)
    return sum(ms) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
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
                r["pyramid_ms"] = per_call_ms(ctx, lambda: ctx.motion_pyramid(p, c, m, 2, 16, 2), a.calls, a.warmup)
                r["full_search_ms"] = per_call_ms(ctx, lambda: ctx.motion(p, c, m), a.calls, a.warmup)
                for est, key in ((capi.ESTIMATOR_PYRAMID, "frames_pyramid_ms"), (capi.ESTIMATOR_FULL_SEARCH, "frames_full_ms")):
                    ctx.set_motion_estimator(est)
                    r[key] = per_call_ms(ctx, lambda: ctx.interpolate_frames(p, c, o, 0.5), a.calls, a.warmup)
                ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
                rows.append(r)
                print(json.dumps(r), flush=True)
                for f in (p, c, m, o):
                    ctx.destroy_frame(f)
    for size in a.sizes.split(","):
        t = [r["pyramid_ms"] for r in rows if r["size"] == size]
        print(json.dumps({"size": size, "pyramid_min_ms": min(t), "pyramid_max_ms": max(t),
                          "pyramid_spread_pct": 100.0 * (max(t) - min(t)) / min(t)}))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
