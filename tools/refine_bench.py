"""Time lfg_motion_refine at radius 0, 1 and 2, at 1080p, 4K and 8K on four vector fields: a pan (lfg_motion's vectors under
the intended semantics), moving objects over a panned background (lfg_motion_pyramid's), uncorrelated frames (lfg_motion's)
and dense random vectors.  Device-event timing (lfg_profile_*: HIP events around every stage launch), 200 calls after 20 of
warm-up by default.

    python tools/refine_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json]
"""
from __future__ import annotations

import numpy as np

from stage_bench import SIZES, arguments, emit, per_call_ms, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402

RADII = [0, 1, 2]


def moving_objects(w, h, seed=11):
    """A synth background panned by (4, -2) and 24 textured squares of 24 to 160 px, each moving by its own vector."""
    rng = np.random.default_rng(seed)
    bg = synth.make_prev(w, h)
    prev, curr = bg.copy(), synth.translate(bg, (4, -2))
    for _ in range(24):
        size = int(rng.integers(24, 161))
        sx, sy = (int(v) for v in rng.integers(-30, 31, 2))
        x, y = int(rng.integers(40, w - size - 40)), int(rng.integers(40, h - size - 40))
        tex = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
        prev[y:y + size, x:x + size] = tex
        curr[y + sy:y + sy + size, x + sx:x + sx + size] = tex
    return prev, curr


def contents(w, h):
    """(name, prev, curr, vectors or the estimator that makes them)"""
    prev = synth.make_prev(w, h)
    yield "pan(6,-4)", prev, synth.translate(prev, (6, -4)), "full"
    a, b = moving_objects(w, h)
    yield "moving-objects", a, b, "pyramid"
    a, b = synth.make_uncorrelated_pair(w, h)
    yield "uncorrelated", a, b, "full"
    yield "random-mv", a, b, np.random.default_rng(5).integers(-128, 128, (h, w, 2)).astype(np.int8)


def per_call_us(ctx, fn, calls, warmup):
    return 1000.0 * per_call_ms(ctx, fn, calls, warmup, capi.STAGE_MOTION)


def main():
    a = arguments("1080p,4k,8k")
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr, vectors in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                if isinstance(vectors, str):
                    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                    if vectors == "full":
                        ctx.motion(p, c, m)
                    else:
                        ctx.motion_pyramid(p, c, m, 2, 16, 2)
                else:
                    m = ctx.frame_from(vectors, capi.FORMAT_MV_S8X2)
                o = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                ctx.sync()
                mv = ctx.download(m)
                # the share of pixels whose 17 candidates are not all equal (the lanes that do cost work)
                # (edge-padded: near the image's edges an approximation)
                pad = np.pad(mv, ((8, 8), (8, 8), (0, 0)), mode="edge")
                mixed = np.zeros((h, w), bool)
                for dx, dy in [(i * s, j * s) for s in (4, 8) for j in (-1, 0, 1) for i in (-1, 0, 1)]:
                    mixed |= (pad[8 + dy:8 + dy + h, 8 + dx:8 + dx + w] != mv).any(-1)
                r = {"size": size, "content": name, "mixed_share": round(float(mixed.mean()), 4)}
                for radius in RADII:
                    r[f"r{radius}_us"] = per_call_us(ctx, lambda: ctx.motion_refine(p, c, m, o, radius), a.calls, a.warmup)
                emit(rows, r)
                for f in (p, c, m, o):
                    ctx.destroy_frame(f)
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
