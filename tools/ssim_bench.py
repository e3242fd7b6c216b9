"""Time the structural similarity: lfg_frame_ssim at 1080p, 4K and 8K on five contents -- identical frames, b = a +- 1 on random
channels, unrelated frames, 0 against 255, a checkerboard against its inverse -- through both load paths (16-byte: frames as
lfg_frame_create makes them; dword: the same pixels in frames one pixel wider, whose pitch is no multiple of 16) and with
accumulate 0 and 1.  In the same run, as the yardstick, lfg_frame_diff on the same frames: both calls read 8 bytes per pixel and
write a record.  Neither call is under a stage timer, so the HIP events go around every call: 200 calls after 20 of warm-up.

    python tools/ssim_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and the kernel's resources (read from the code object's notes), as
profiles/ssim_4k_profile.txt keeps them.
"""
from __future__ import annotations

import hashlib
import json
import sys

import numpy as np

from stage_bench import SIZES, emit, write_json                # (puts the repository root on sys.path)
from diff_bench import HBM_PEAK, Events, kernel_resources, padded
from linux_fg_amd import capi, synth  # noqa: E402


def contents(w, h):
    """(name, a, b) as host arrays."""
    a = synth.make_prev(w, h)
    yield "identical", a, a
    rng = np.random.default_rng(3)
    step = np.zeros((h, w, 4), np.int16)
    np.put_along_axis(step, rng.integers(0, 4, (h, w, 1)), rng.choice([-1, 1], size=(h, w, 1)).astype(np.int16), axis=-1)
    yield "+-1", a, np.clip(a.astype(np.int16) + step, 0, 255).astype(np.uint8)
    yield "unrelated", rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yield "0-against-255", np.zeros((h, w, 4), np.uint8), np.full((h, w, 4), 255, np.uint8)
    yy, xx = np.mgrid[:h, :w]
    board = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 4, axis=-1)
    yield "checkerboard-against-inverse", board, 255 - board


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k,8k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            pixels = w * h
            r, d = ctx.create_ssim_record(), ctx.create_diff_record()
            for name, x, y in contents(w, h):
                fx, fy = ctx.frame_from(x), ctx.frame_from(y)
                bx, vx = padded(ctx, x)
                by, vy = padded(ctx, y)
                for path, (fa, fb) in (("16-byte", (fx, fy)), ("dword", (vx, vy))):
                    ctx.frame_ssim(fa, fb, r)
                    record = ctx.read_ssim_record(r)
                    s = capi.summarize_ssim(record)
                    row = {"part": "frame_ssim", "size": size, "content": name, "loads": path, "ssim": s["all"],
                           "identical": s["identical"], "below_half": s["below_half"], "bins": sum(1 for v in record[2] if v)}
                    for label, acc in (("write", False), ("accumulate", True)):
                        med, mean = events.per_call_us(ctx, lambda: ctx.frame_ssim(fa, fb, r, 0xF, acc), a.warmup)
                        row[f"{label}_median_us"], row[f"{label}_mean_us"] = med, mean
                    diff_us, diff_mean = events.per_call_us(ctx, lambda: ctx.frame_diff(fa, fb, d), a.warmup)
                    row["frame_diff_median_us"], row["frame_diff_mean_us"] = diff_us, diff_mean
                    row["share_of_8TBps"] = 8 * pixels / (row["write_median_us"] * 1e-6) / HBM_PEAK
                    row["of_frame_diff"] = row["write_median_us"] / diff_us
                    emit(rows, row)
                for f in (fx, fy, bx, by):
                    ctx.destroy_frame(f)
            ctx.destroy_frame(r)
            ctx.destroy_frame(d)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/ssim_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; share_of_8TBps = 8 bytes per pixel over the median, as a share of 8 TB/s;\n"
                    "# of_frame_diff = the call's median over lfg_frame_diff's on the same frames in the same run.\n")
            for kernel, text in kernel_resources("frame_ssim_kernel").items():
                f.write(f"# frame_ssim_kernel<{kernel}>: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
