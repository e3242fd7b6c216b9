"""Time half-resolution motion next to the full-resolution estimators, at 1080p and 4K on pyramid_bench.py's five contents:
lfg_motion_pyramid(2, 16, 2) and lfg_motion(8, 16) on the pair, the half-resolution route of each (lfg_frame_halve twice, the
estimator on the halves -- lfg_motion_pyramid(1, 16, 2) or lfg_motion(8, 16) -- and lfg_motion_expand) at radius 0, 1 and 2,
and lfg_motion_expand alone.  Device-event timing (lfg_profile_*: HIP events around every stage launch): one sample per call,
200 calls after 20 of warm-up by default, medians.  Each full-resolution call is timed before and after its routes; the
distance between its two medians is the run's spread.

    python tools/expand_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--json out.json]
"""
from __future__ import annotations

import statistics

from pyramid_bench import contents
from stage_bench import SIZES, arguments, emit, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi  # noqa: E402

RADII = [0, 1, 2]
MV = capi.FORMAT_MV_S8X2


def median_ms(ctx, fn, calls, warmup):
    """The median over `calls` calls of fn() of the milliseconds its motion-stage launches took on the device."""
    for _ in range(warmup):
        fn()
    ctx.sync()
    ctx.profile_enable(True)
    samples = []
    for _ in range(calls):
        ctx.profile_reset()
        fn()
        samples.append(ctx.profile_get(capi.STAGE_MOTION)[0])
    ctx.profile_enable(False)
    return statistics.median(samples)


def main():
    a = arguments("1080p,4k")
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            wl, hl = (w + 1) // 2, (h + 1) // 2
            for name, prev, curr in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                m = ctx.create_frame(w, h, MV)
                hp, hc, low = ctx.create_frame(wl, hl), ctx.create_frame(wl, hl), ctx.create_frame(wl, hl, MV)

                def route(estimate, radius):
                    ctx.frame_halve(p, hp)
                    ctx.frame_halve(c, hc)
                    estimate(hp, hc, low)
                    ctx.motion_expand(p, c, low, m, radius)

                t = lambda fn: round(median_ms(ctx, fn, a.calls, a.warmup), 4)
                r = {"size": size, "content": name}
                for key, full, half in (("pyramid", lambda: ctx.motion_pyramid(p, c, m, 2, 16, 2), lambda x, y, z: ctx.motion_pyramid(x, y, z, 1, 16, 2)),
                                        ("full_search", lambda: ctx.motion(p, c, m), lambda x, y, z: ctx.motion(x, y, z))):
                    r[f"{key}_before_ms"] = t(full)
                    for radius in RADII:
                        r[f"{key}_half_r{radius}_ms"] = t(lambda: route(half, radius))
                    if key == "pyramid":                         # `low` now holds the half-size pyramid's field
                        for radius in RADII:
                            r[f"expand_r{radius}_ms"] = t(lambda: ctx.motion_expand(p, c, low, m, radius))
                    r[f"{key}_after_ms"] = t(full)
                    r[f"{key}_spread_ms"] = round(abs(r[f"{key}_after_ms"] - r[f"{key}_before_ms"]), 4)
                emit(rows, r)
                for f in (p, c, m, hp, hc, low):
                    ctx.destroy_frame(f)
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
