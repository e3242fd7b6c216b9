"""Time lfg_upscale_edge, 1080p -> 4K and 1080p -> 1440p, and in the same run, as the yardsticks, lfg_resample under Lanczos-3 and
Catmull-Rom and lfg_scale on the same frames -- never a stored number.  HIP events go around every call: 200 calls after 20 of
warm-up, medians.  Each yardstick is timed before and after the edge-adaptive call: its two medians show the run-to-run spread
next to the quotient.  Every call works on the same buffers again, so they are served from the 256 MiB Infinity Cache: rates, no
HBM figures; the quotient compares like with like.

The frame is a scene of bars and discs at random angles over a smooth background, rendered with analytic coverage at the input
size and again at the output size: the second rendering is the truth, and each result's PSNR (lfg_frame_diff) and SSIM
(lfg_frame_ssim) against it, over R, G and B, are the library's own figures.

    python tools/edge_bench.py [--calls 200] [--warmup 20] [--seed 0] [--json out.json] [--out profile.txt]
    python tools/edge_bench.py --drive 1080p->4k --calls 50          # that many calls and nothing else: what a profiler is put around

--out writes the rows, stamped with the library's sha and the kernel's resources (read from the code object's notes), as
profiles/edge_4k_profile.txt keeps them.
"""
from __future__ import annotations

import hashlib
import json

import numpy as np

from diff_bench import Events, kernel_resources              # (stage_bench, imported there, puts the repository root on sys.path)
from stage_bench import emit, write_json
from linux_fg_amd import capi  # noqa: E402

PAIRS = (("1080p->4k", (1920, 1080), (3840, 2160)), ("1080p->1440p", (1920, 1080), (2560, 1440)))
RGB = 0x7


def render(w, h, seed, shapes=40):
    """The scene at w x h: every shape is given in units of the frame's height and covers a pixel by its distance to the
    shape's outline, clamped to one pixel -- what a box filter over the pixel gives for a straight outline."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    x, y = (x + 0.5) / h, (y + 0.5) / h                              # the frame is w / h wide and 1 high
    img = np.stack([96 + 48 * np.sin(3 * x + ph) * np.cos(2 * y + ph) for ph in rng.uniform(0, 6, 3)], -1).astype(np.float32)
    for _ in range(shapes):
        cx, cy, colour = rng.uniform(0, w / h), rng.uniform(0, 1), rng.uniform(0, 255, 3).astype(np.float32)
        if rng.integers(0, 2):
            cover = np.clip(0.5 + (rng.uniform(1 / 64, 1 / 8) - np.hypot(x - cx, y - cy)) * h, 0, 1)
        else:
            angle, half, length = rng.uniform(0, np.pi), rng.uniform(1 / 400, 1 / 40), rng.uniform(1 / 10, 1 / 2)
            u, v = (x - cx) * np.cos(angle) + (y - cy) * np.sin(angle), -(x - cx) * np.sin(angle) + (y - cy) * np.cos(angle)
            cover = np.clip(0.5 + (half - np.abs(v)) * h, 0, 1) * np.clip(0.5 + (length - np.abs(u)) * h, 0, 1)
        img += cover[..., None].astype(np.float32) * (colour - img)
    return np.concatenate([np.rint(img), np.full((h, w, 1), 255.0, np.float32)], -1).astype(np.uint8)


def quality(ctx, got, truth, diff_record, ssim_record):
    ctx.frame_diff(got, truth, diff_record, RGB)
    ctx.frame_ssim(got, truth, ssim_record, RGB)
    d, s = capi.summarize(ctx.read_diff_record(diff_record), RGB), capi.summarize_ssim(ctx.read_ssim_record(ssim_record), RGB)
    return {"psnr_db": d["psnr_db"], "ssim": s["all"], "ssim_db": s["db"]}


def drive(pair, calls, seed):
    (w, h), (ow, oh) = next((i, o) for p, i, o in PAIRS if p == pair)
    with capi.Context(0) as ctx:
        src, dst = ctx.frame_from(render(w, h, seed)), ctx.create_frame(ow, oh)
        for _ in range(calls):
            ctx.upscale_edge(src, dst)
        ctx.sync()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--drive", default=None, metavar="PAIR")
    a = ap.parse_args()
    if a.drive:
        return drive(a.drive, a.calls, a.seed)
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        diff_record, ssim_record = ctx.create_diff_record(), ctx.create_ssim_record()
        for pair, (w, h), (ow, oh) in PAIRS:
            src, truth, dst = ctx.frame_from(render(w, h, a.seed)), ctx.frame_from(render(ow, oh, a.seed)), ctx.create_frame(ow, oh)
            yardsticks = (("lfg_resample lanczos3", lambda: ctx.resample(src, dst, capi.FILTER_LANCZOS3)),
                          ("lfg_resample catmull-rom", lambda: ctx.resample(src, dst, capi.FILTER_CATMULL_ROM)),
                          ("lfg_scale", lambda: ctx.scale(src, dst)))
            before = {}
            for name, call in yardsticks:
                before[name] = events.per_call_us(ctx, call, a.warmup)[0]
            med, mean = events.per_call_us(ctx, lambda: ctx.upscale_edge(src, dst), a.warmup)
            emit(rows, {"pair": pair, "call": "lfg_upscale_edge", "median_us": med, "mean_us": mean, "pixels_per_us": ow * oh / med,
                        **quality(ctx, dst, truth, diff_record, ssim_record)})
            for name, call in yardsticks:
                after = events.per_call_us(ctx, call, a.warmup)[0]
                emit(rows, {"pair": pair, "call": name, "median_us_before": before[name], "median_us_after": after,
                            "edge_over_this": med / ((before[name] + after) / 2), **quality(ctx, dst, truth, diff_record, ssim_record)})
            for f in (src, truth, dst):
                ctx.destroy_frame(f)
        ctx.destroy_frame(diff_record)
        ctx.destroy_frame(ssim_record)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/edge_bench.py --calls {a.calls} --warmup {a.warmup} --seed {a.seed}: HIP events around every call, {a.calls} calls\n"
                    f"# after {a.warmup} of warm-up, medians in us.  edge_over_this = lfg_upscale_edge's median over the mean of the yardstick's two\n"
                    "# medians of the same run (same frames; taken before and after: their distance is the spread).  The buffers stay in the\n"
                    "# 256 MiB Infinity Cache: rates, no HBM figure.  psnr_db (lfg_frame_diff), ssim and ssim_db (lfg_frame_ssim) are over R, G, B\n"
                    "# against the scene rendered at the output size.\n")
            for text in kernel_resources("upscale_edge_kernel").values():
                f.write(f"# upscale_edge_kernel: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
