"""Time and judge quarter-pixel vectors, at 1080p and 4K on an integer pan, a fractional pan and
uncorrelated frames:
  * lfg_motion_subpel at radius 0, 1 and 2 -- the stage does the same work on every content, so the three should agree;
  * lfg_interpolate_compensated_subpel next to lfg_interpolate_compensated in the same run, on the same frames, the
    sub-pixel call on 4 * the integer field (the same bytes out) and on the refined field;
  * quality through the project's own interface: lfg_host --evaluate --input-raw on a stream this tool writes, with and
    without --subpel-vectors R, on the fractional pan and on the integer pan, where the two must agree.
Device-event timing (lfg_profile_*: HIP events around every stage launch): one sample per call, 100 calls after 20 of warm-up
by default, medians.  The integer route is timed before and after the sub-pixel one; the distance between its two medians is
the run's spread.

    python tools/subpel_bench.py [--calls 100] [--warmup 20] [--sizes 1080p,4k] [--json out.json] [--no-quality | --quality-only]
"""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

from stage_bench import SIZES, emit, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi  # noqa: E402

RADII = [0, 1, 2]
MV, MVQ = capi.FORMAT_MV_S8X2, capi.FORMAT_MV_S16X2_Q2
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "linux-fg_amd", "lfg_host")
PAD = 40                                              # frame pixels of master around the frame


def pan_frames(w, h, offsets, cell=8, seed=7):
    """tests/subpel_cases.py's scene at any size: the rounded 4 x 4 box means of a master of random bytes on cell x cell cells
    at the quarter-pixel `offsets`, made in strips of 64 rows so that the 4 x master never exists as a whole."""
    rng = np.random.default_rng(seed)
    mh, mw = (h + 2 * PAD) * 4, (w + 2 * PAD) * 4
    coarse = rng.integers(0, 256, (mh // cell + 2, mw // cell + 2, 4)).astype(np.uint16)
    out = []
    for ox, oy in offsets:
        frame = np.empty((h, w, 4), np.uint8)
        for r0 in range(0, h, 64):
            rows = min(64, h - r0)
            ys = (PAD * 4 + oy + r0 * 4 + np.arange(rows * 4)) // cell
            xs = (PAD * 4 + ox + np.arange(w * 4)) // cell
            strip = coarse[ys][:, xs]
            frame[r0:r0 + rows] = ((strip.reshape(rows, 4, w, 4, 4).sum(axis=(1, 3), dtype=np.uint32) + 8) >> 4).astype(np.uint8)
        out.append(frame)
    return out


def contents(w, h):
    """(name, prev, curr, integer vectors): a pan by whole pixels, one by (2.5, -1.5) px, and frames that share nothing."""
    a, b = pan_frames(w, h, [(0, 0), (8, -8)])
    yield "integer_pan", a, b, (2, -2)
    a, b = pan_frames(w, h, [(0, 0), (10, -6)])
    yield "fractional_pan", a, b, (3, -1)
    rng = np.random.default_rng(11)
    yield "uncorrelated", rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8), (0, 0)


def median_ms(ctx, fn, calls, warmup, stage):
    for _ in range(warmup):
        fn()
    ctx.sync()
    ctx.profile_enable(True)
    samples = []
    for _ in range(calls):
        ctx.profile_reset()
        fn()
        samples.append(ctx.profile_get(stage)[0])
    ctx.profile_enable(False)
    return statistics.median(samples)


def evaluate(raw, w, h, frames, extra):
    p = subprocess.run([HOST, "--input-width", str(w), "--input-height", str(h), "--frames", str(frames), "--quiet", "--evaluate",
                        "--input-raw", raw, "--motion", "pyramid", "--interpolator", "compensated", "--semantics", "intended", *extra],
                       capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise SystemExit(f"lfg_host failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])["evaluation"]


def quality(rows, w, h):
    """Frames 0, 2, 4 are the stream and 1, 3 are held out: a pan of `step` quarter pixels per frame, over 8 px cells.  (The
    tests' 2 px cells are the sharpest content there is: a pair whose first frame sits on the cell grid is reproduced exactly
    by bilinear samples, any later pair of the same stream is aliasing that no vector explains -- on such a stream the second
    pair's gate passes 2 % of the pixels with the TRUE vectors.  A stream has to be band-limited to say anything.)"""
    with tempfile.TemporaryDirectory() as tmp:
        for name, step in (("fractional_pan", (5, -3)), ("integer_pan", (4, -4))):
            raw = os.path.join(tmp, name + ".rgba")
            np.concatenate([f.reshape(-1) for f in pan_frames(w, h, [(k * step[0], k * step[1]) for k in range(5)], cell=32)]).tofile(raw)
            emit(rows, {"quality": name, "size": f"{w}x{h}", "subpel_vectors": -1, "evaluation": evaluate(raw, w, h, 5, [])})
            for radius in RADII:
                emit(rows, {"quality": name, "size": f"{w}x{h}", "subpel_vectors": radius,
                            "evaluation": evaluate(raw, w, h, 5, ["--subpel-vectors", str(radius)])})


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        for size in [] if a.quality_only else a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr, v in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                mv = np.zeros((h, w, 2), np.int8)
                mv[...] = v
                m, q4 = ctx.frame_from(mv, MV), ctx.frame_from(4 * mv.astype(np.int16), MVQ)
                q, o = ctx.create_frame(w, h, MVQ), ctx.create_frame(w, h)
                t = lambda fn, stage: round(median_ms(ctx, fn, a.calls, a.warmup, stage), 4)
                r = {"size": size, "content": name}
                for radius in RADII:
                    r[f"subpel_r{radius}_ms"] = t(lambda: ctx.motion_subpel(p, c, m, q, radius), capi.STAGE_MOTION)
                ctx.motion_subpel(p, c, m, q, 1)
                r["compensated_before_ms"] = t(lambda: ctx.interpolate_compensated(p, c, m, o, 0.5, 48), capi.STAGE_INTERPOLATE)
                r["subpel_route_4mv_ms"] = t(lambda: ctx.interpolate_compensated_subpel(p, c, q4, o, 0.5, 48), capi.STAGE_INTERPOLATE)
                r["subpel_route_refined_ms"] = t(lambda: ctx.interpolate_compensated_subpel(p, c, q, o, 0.5, 48), capi.STAGE_INTERPOLATE)
                r["compensated_after_ms"] = t(lambda: ctx.interpolate_compensated(p, c, m, o, 0.5, 48), capi.STAGE_INTERPOLATE)
                r["compensated_spread_ms"] = round(abs(r["compensated_after_ms"] - r["compensated_before_ms"]), 4)
                emit(rows, r)
                for f in (p, c, m, q4, q, o):
                    ctx.destroy_frame(f)
    if not a.no_quality:
        quality(rows, 1920, 1080)
    write_json(a.json, rows)


if __name__ == "__main__":
    sys.exit(main())
