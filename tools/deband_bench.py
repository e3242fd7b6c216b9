"""Time lfg_deband: 1080p and 4K; I = 1 and I = 4, each at R = 16 and R = 32, at T = 4 and G = 3 (the cost depends on neither, nor
on the content: the kernel has no data-dependent branch) on a gradient scene; through the 16-byte kernel (frames as
lfg_frame_create makes them) and, at R = 16, through the dword kernel alone (pitches that are no multiple of 16).  In the same
run, as the yardstick, lfg_sharpen at strength 16 on the same frame, timed before and after the deband rows of a size: the
quotient of the two is the run's own spread, against which every other difference is read.  The call is outside the stage timers,
so the HIP events go around every call here: 200 calls after 20 of warm-up, medians.  Every call works on the same buffers again,
so they are served from the 256 MiB Infinity Cache, as the yardstick's are: the quotient compares like with like.

    python tools/deband_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--json out.json] [--out profile.txt]
    python tools/deband_bench.py --drive 4k:4:16 --calls 50         # that many calls at size:I:R and nothing else: what a profiler is put around

--out writes the rows, stamped with the library's sha and the kernels' resources (read from the code object's notes), as
profiles/deband_4k_profile.txt keeps them.
"""
from __future__ import annotations

import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

from diff_bench import Events                                 # (stage_bench, imported there, puts the repository root on sys.path)
from stage_bench import SIZES, emit, write_json
from linux_fg_amd import capi  # noqa: E402

SETTINGS = ((1, 16), (1, 32), (4, 16), (4, 32))               # (iterations, radius)
THRESHOLD, GRAIN, SHARPEN = 4, 3, 16


def kernel_resources():
    """{"I=.. wide / dword": "vgprs ..., sgprs ..., lds ..., scratch ..., waves/SIMD ..."} of the deband kernels, from the notes of
    the library's code objects (llvm-objdump --offloading unbundles them into the working directory, here a temporary one)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(capi.LIB_PATH, d)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=d, capture_output=True, text=True)
        for f in sorted(glob.glob(os.path.join(d, "*gfx950*"))):
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+\S*deband_kernelILi(\d)ELb(\d)E\S*", block)
                if not name:
                    continue
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block)[1])  # noqa: E731
                vgprs = get("vgpr_count")
                found[f"I={name[1]} {'wide' if name[2] == '1' else 'dword'}"] = (
                    f"vgprs {vgprs}, sgprs {get('sgpr_count')}, lds {get('group_segment_fixed_size')} B, scratch "
                    f"{get('private_segment_fixed_size')} B, waves/SIMD {min(8, 512 // (-(-vgprs // 8) * 8))} by registers")
    return found


def gradient_scene(w, h):
    """Slow ramps per channel, rounded: bands a few pixels wide and wider, what the call is for."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    frame = np.empty((h, w, 4), np.uint8)
    for c, (ax, ay, base) in enumerate(((0.011, 0.005, 60.0), (0.004, 0.017, 120.0), (-0.007, 0.009, 200.0))):
        frame[..., c] = np.clip(np.rint(base + ax * xs + ay * ys), 0, 255).astype(np.uint8)
    frame[..., 3] = 255
    return frame


def drive(what, calls):
    size, iterations, radius = what.split(":")
    w, h = SIZES[size]
    with capi.Context(0) as ctx:
        src, dst = ctx.frame_from(gradient_scene(w, h)), ctx.create_frame(w, h)
        for seed in range(calls):
            ctx.deband(src, dst, int(iterations), THRESHOLD, int(radius), GRAIN, seed)
        ctx.sync()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--drive", default=None, metavar="SIZE:I:R")
    a = ap.parse_args()
    if a.drive:
        return drive(a.drive, a.calls)
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            frame, out = ctx.frame_from(gradient_scene(w, h)), ctx.create_frame(w, h)
            odd_in, odd_out = ctx.create_frame(w + 1, h), ctx.create_frame(w + 1, h)      # pitches that are no multiple of 16
            odd_src, odd_dst = (capi.Context.wrap(f.data, w, h, pitch=f.pitch) for f in (odd_in, odd_out))
            ctx.copy(frame, odd_src)

            def sharpen(part):
                med, mean = events.per_call_us(ctx, lambda: ctx.sharpen(frame, out, SHARPEN), a.warmup)
                emit(rows, {"part": part, "size": size, "call": f"lfg_sharpen, strength {SHARPEN}", "path": "16-byte", "median_us": med, "mean_us": mean})
                return med

            before = sharpen("yardstick, before")
            seed = 0
            for path, src, dst, settings in (("16-byte", frame, out, SETTINGS), ("dword", odd_src, odd_dst, ((1, 16), (4, 16)))):
                for iterations, radius in settings:
                    def call():
                        nonlocal seed
                        seed += 1                              # the presented-frame counter, as the host loop passes it
                        ctx.deband(src, dst, iterations, THRESHOLD, radius, GRAIN, seed)
                    med, mean = events.per_call_us(ctx, call, a.warmup)
                    emit(rows, {"part": "deband", "size": size, "path": path, "iterations": iterations, "radius": radius, "threshold": THRESHOLD,
                                "grain": GRAIN, "median_us": med, "mean_us": mean, "gathered_dwords_per_pixel": 4 * iterations,
                                "of_sharpen": med / before})
            after = sharpen("yardstick, after")
            emit(rows, {"part": "spread", "size": size, "sharpen_after_over_before": after / before})
            for f in (frame, out, odd_in, odd_out):
                ctx.destroy_frame(f)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/deband_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; of_sharpen = the call's median over lfg_sharpen's (strength 16, 16-byte route, same\n"
                    "# frame, timed before the deband rows of the size); sharpen_after_over_before = the yardstick timed again behind them,\n"
                    "# the run's own spread.  Every call works on the same buffers again, and they stay in the 256 MiB Infinity Cache, as\n"
                    "# the yardstick's do.\n")
            for kernel, text in sorted(kernel_resources().items()):
                f.write(f"# deband_kernel<{kernel}>: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
