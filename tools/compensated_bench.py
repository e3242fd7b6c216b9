"""Time lfg_interpolate_compensated next to the shader's lfg_interpolate, with one factor and with three (t = 1/4, 1/2, 3/4),
at 1080p, 4K and 8K on five contents.  Device-event timing (lfg_profile_*: HIP events around every stage launch), after
warm-up; the vectors come from lfg_motion under the intended semantics, except for the dense random field.

    python tools/compensated_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json]
"""
from __future__ import annotations

import numpy as np

from stage_bench import SIZES, arguments, emit, per_call_ms, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402

FACTORS = [0.25, 0.5, 0.75]


def contents(w, h):
    """(name, prev, curr, vectors or None for lfg_motion's, match_sad)"""
    prev = synth.make_prev(w, h)
    yield "pan(6,-4)", prev, synth.translate(prev, (6, -4)), None, 48
    sq = prev.copy()                                        # a 256 x 256 block of prev moved by (12, 0) over the still rest
    x, y = w // 2 - 128, h // 2 - 128
    sq[y:y + 256, x + 12:x + 268] = prev[y:y + 256, x:x + 256]
    yield "square(12,0)", prev, sq, None, 48
    a, b = synth.make_uncorrelated_pair(w, h)
    yield "uncorrelated", a, b, None, 48
    rng = np.random.default_rng(5)
    yield "random-mv,sad1020", a, b, rng.integers(-128, 128, (h, w, 2)).astype(np.int8), 1020
    yield "static", prev, prev.copy(), None, 48


def per_call_us(ctx, fn, calls, warmup):
    return 1000.0 * per_call_ms(ctx, fn, calls, warmup, capi.STAGE_INTERPOLATE)


def main():
    a = arguments("1080p,4k,8k")
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr, vectors, ms in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                if vectors is None:
                    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                    ctx.motion(p, c, m)
                else:
                    m = ctx.frame_from(vectors, capi.FORMAT_MV_S8X2)
                outs = [ctx.create_frame(w, h) for _ in FACTORS]
                r = {"size": size, "content": name, "match_sad": ms}
                r["shader_us"] = per_call_us(ctx, lambda: ctx.interpolate(p, c, m, outs[0], 0.5), a.calls, a.warmup)
                r["compensated_us"] = per_call_us(ctx, lambda: ctx.interpolate_compensated(p, c, m, outs[0], 0.5, ms), a.calls, a.warmup)
                r["shader_x3_us"] = per_call_us(ctx, lambda: ctx.interpolate_multi(p, c, m, outs, FACTORS), a.calls, a.warmup)
                r["compensated_x3_us"] = per_call_us(ctx, lambda: ctx.interpolate_compensated_multi(p, c, m, outs, FACTORS, ms),
                                                     a.calls, a.warmup)
                emit(rows, r)
                for f in [p, c, m] + outs:
                    ctx.destroy_frame(f)
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
