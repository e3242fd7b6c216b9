"""Time and weigh level matching (lfg_frame_histogram, lfg_levels_match, lfg_levels_apply, lfg_set_level_matching), four parts:

  histogram  lfg_frame_histogram at 1080p and 4K on flat, ramp, noise and the bench's pan content, through both load paths, beside
             lfg_frame_diff(a, a) on the same frame: the same bytes read once more, and one 256-bin histogram instead of four.
  apply      lfg_levels_apply in both modes, in place and out of place, beside lfg_frame_copy of the same frame.
  whole      lfg_interpolate_frames_multi (compensated, intended semantics, factors 0.5) at 4K with the pyramid and with the full
             search, on a plain pan and on the same pan faded by 205 / 256, with the switch off, at 32 and at 0: HIP events
             around the call, and the motion and interpolate stage timers (the levelling calls are outside both).
  quality    a 1080p pan that fades out and in, one with a two-frame flash and a plain pan: every second frame is held out,
             generated at 0.5 from its neighbours (compensated, pyramid, cut detection at 500) and compared on the GPU
             (lfg_frame_diff, lfg_frame_ssim), with the switch off and at 32; the pairs reported as cuts and as levelled.

    python tools/levels_bench.py [--calls 200] [--warmup 20] [--parts histogram,apply,whole,quality] [--json out.json]

Every comparison is taken in one run; medians of HIP-event times over the calls.
"""
from __future__ import annotations

import argparse

import numpy as np

from stage_bench import SIZES, emit, per_call_ms, write_json        # (puts the repository root on sys.path)
from diff_bench import Events, padded
from linux_fg_amd import capi, synth  # noqa: E402

THRESHOLD = 32
PAN = (3, -2)


def fade(frame, gain, offset=0):
    out = frame.copy()
    out[..., :3] = np.clip(((frame[..., :3].astype(np.int32) * gain + 128) >> 8) + offset, 0, 255).astype(np.uint8)
    return out


def histogram_contents(w, h):
    yield "flat", np.full((h, w, 4), (90, 140, 200, 255), np.uint8)
    x = (np.arange(w) % 256).astype(np.uint8)
    yield "ramp", np.broadcast_to(np.stack([x, 255 - x, x ^ 0x55, (x + 128).astype(np.uint8)], -1), (h, w, 4)).copy()
    yield "noise", np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8)
    yield "bench-pan", synth.translate(synth.make_prev(w, h), PAN)


def part_histogram(ctx, events, a, rows):
    for size in ("1080p", "4k"):
        w, h = SIZES[size]
        rec, diff = ctx.create_histogram_record(), ctx.create_diff_record()
        for name, host in histogram_contents(w, h):
            f = ctx.frame_from(host)
            big, view = padded(ctx, host)
            for path, frame in (("16-byte", f), ("dword", view)):
                ctx.frame_histogram(frame, rec)
                pixels, hist = ctx.read_histogram_record(rec)
                want = np.stack([np.bincount(host[..., c].reshape(-1), minlength=256) for c in range(4)])
                assert pixels == w * h and (hist == want).all(), (size, name, path)
                med, mean = events.per_call_us(ctx, lambda: ctx.frame_histogram(frame, rec), a.warmup)
                dmed, _ = events.per_call_us(ctx, lambda: ctx.frame_diff(frame, frame, diff), a.warmup)
                emit(rows, {"part": "histogram", "size": size, "content": name, "loads": path, "median_us": med, "mean_us": mean,
                            "frame_diff_a_a_median_us": dmed, "GBps": 4 * w * h / med / 1e3, "bins": int((hist > 0).sum())})
            ctx.destroy_frame(f)
            ctx.destroy_frame(big)
        ctx.destroy_frame(rec)
        ctx.destroy_frame(diff)


def part_apply(ctx, events, a, rows):
    for size in ("1080p", "4k"):
        w, h = SIZES[size]
        prev = synth.make_prev(w, h)
        curr = fade(synth.translate(prev, PAN), 205)
        p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
        ra, rb, m = ctx.create_histogram_record(), ctx.create_histogram_record(), ctx.create_levels_map()
        ctx.frame_histogram(p, ra)
        ctx.frame_histogram(c, rb)
        ctx.levels_match(ra, rb, m, 0)
        assert ctx.read_levels_map(m)["active"] == 1
        copy_us, _ = events.per_call_us(ctx, lambda: ctx.copy(p, o), a.warmup)
        match_us, _ = events.per_call_us(ctx, lambda: ctx.levels_match(ra, rb, m, 0), a.warmup)
        emit(rows, {"part": "apply", "size": size, "call": "lfg_frame_copy", "median_us": copy_us})
        emit(rows, {"part": "apply", "size": size, "call": "lfg_levels_match", "median_us": match_us})
        for label, mode, factor in (("forward", capi.LEVELS_FORWARD, 0.0), ("at 0.5", capi.LEVELS_AT, 0.5)):
            out_us, _ = events.per_call_us(ctx, lambda: ctx.levels_apply(p, o, m, mode, factor), a.warmup)
            in_us, _ = events.per_call_us(ctx, lambda: ctx.levels_apply(o, o, m, mode, factor), a.warmup)
            emit(rows, {"part": "apply", "size": size, "call": f"lfg_levels_apply {label}", "median_us": out_us, "in_place_median_us": in_us,
                        "of_copy": out_us / copy_us, "GBps": 8 * w * h / out_us / 1e3})
        for f in (p, c, o, ra, rb, m):
            ctx.destroy_frame(f)


def part_whole(ctx, events, a, rows):
    w, h = SIZES["4k"]
    prev = synth.make_prev(w, h)
    pan = synth.translate(prev, PAN)
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    ctx.set_interpolator(capi.INTERPOLATOR_COMPENSATED)
    p, o = ctx.frame_from(prev), ctx.create_frame(w, h)
    calls = max(a.calls // 4, 10)
    short = Events(ctx, calls)
    for content, curr in (("pan", pan), ("faded pan", fade(pan, 205))):
        c = ctx.frame_from(curr)
        for name, estimator in (("pyramid", capi.ESTIMATOR_PYRAMID), ("full search", capi.ESTIMATOR_FULL_SEARCH)):
            ctx.set_motion_estimator(estimator)
            for shift in (-1, THRESHOLD, 0):
                ctx.set_level_matching(shift)
                fn = lambda: ctx.interpolate_frames_multi(p, c, [o], [0.5])  # noqa: E731
                total, _ = short.per_call_us(ctx, fn, max(a.warmup // 4, 3))
                motion = per_call_ms(ctx, fn, calls, 2, capi.STAGE_MOTION)
                interp = per_call_ms(ctx, fn, calls, 2, capi.STAGE_INTERPOLATE)
                row = {"part": "whole", "size": "4k", "content": content, "estimator": name, "match_levels": shift,
                       "call_median_us": total, "motion_ms": motion, "interpolate_ms": interp}
                if shift >= 0:
                    s, n, active = ctx.last_level_match()
                    row.update(active=active, mean_shift_levels=s / (3.0 * n))
                emit(rows, row)
        ctx.destroy_frame(c)
    ctx.set_level_matching(-1)
    ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
    ctx.set_interpolator(capi.INTERPOLATOR_SHADER)
    ctx.set_semantics(capi.SEMANTICS_REFERENCE)
    for f in (p, o):
        ctx.destroy_frame(f)


def streams(w, h, n=13):
    base = synth.make_prev(w, h)
    frame = lambda k: np.roll(base, (k * PAN[1], k * PAN[0]), axis=(0, 1))  # noqa: E731
    out_in = [256, 256, 230, 205, 180, 150, 120, 150, 180, 205, 230, 256, 256]
    flash = [(256, 0)] * 5 + [(256, 60), (256, 60)] + [(256, 0)] * 6
    yield "fade out and in", [fade(frame(k), out_in[k]) for k in range(n)]
    yield "two-frame flash", [fade(frame(k), *flash[k]) for k in range(n)]
    yield "plain pan", [frame(k) for k in range(n)]


def part_quality(ctx, rows):
    w, h = SIZES["1080p"]
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    ctx.set_interpolator(capi.INTERPOLATOR_COMPENSATED)
    ctx.set_motion_estimator(capi.ESTIMATOR_PYRAMID)
    ctx.set_cut_detection(500)
    out, diff, ssim = ctx.create_frame(w, h), ctx.create_diff_record(), ctx.create_ssim_record()
    for name, frames in streams(w, h):
        device = [ctx.frame_from(f) for f in frames]
        reports = {}
        for shift in (-1, THRESHOLD):
            ctx.set_level_matching(shift)
            cuts = levelled = 0
            first = True
            for k in range(1, len(frames) - 1, 2):              # frame k is held out: generated from k - 1 and k + 1
                ctx.interpolate_frames(device[k - 1], device[k + 1], out, 0.5)
                cuts += ctx.last_pair_stats()[1]
                levelled += ctx.last_level_match()[2] if shift >= 0 else 0
                ctx.frame_diff(out, device[k], diff, 0x7, not first)
                ctx.frame_ssim(out, device[k], ssim, 0x7, not first)
                first = False
            d, s = capi.summarize(ctx.read_diff_record(diff), 0x7), capi.summarize_ssim(ctx.read_ssim_record(ssim), 0x7)
            reports[shift] = {"psnr_db": d["psnr_db"], "ssim": s["all"], "p99": d["p99"], "cuts": cuts, "levelled": levelled}
            emit(rows, {"part": "quality", "size": "1080p", "stream": name, "match_levels": shift, "pairs": (len(frames) - 1) // 2, **reports[shift]})
        if name == "plain pan":
            same = {k: v for k, v in reports[-1].items()} == {k: v for k, v in reports[THRESHOLD].items()}
            emit(rows, {"part": "quality", "stream": name, "identical_report_with_and_without": same})
            assert same
        for f in device:
            ctx.destroy_frame(f)
    ctx.set_level_matching(-1)
    ctx.set_cut_detection(-1)
    for f in (out, diff, ssim):
        ctx.destroy_frame(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parts", default="histogram,apply,whole,quality")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        parts = a.parts.split(",")
        if "histogram" in parts:
            part_histogram(ctx, events, a, rows)
        if "apply" in parts:
            part_apply(ctx, events, a, rows)
        if "whole" in parts:
            part_whole(ctx, events, a, rows)
        if "quality" in parts:
            part_quality(ctx, rows)
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
