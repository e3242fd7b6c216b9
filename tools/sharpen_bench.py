"""Time lfg_sharpen: 1080p, 4K and 8K; flat content, a `synth` frame of half the size upscaled by lfg_scale (what the host loop
sharpens) and uniform noise; strengths 0, 16 and 64; through the 16-byte kernel (frames as lfg_frame_create makes them), through
the 16-byte kernel with the dword kernel's remainder launch behind it (the same frames, one column narrower) and through the
dword kernel alone (pitches that are no multiple of 16).  In the same run, as the yardstick, lfg_interpolate on static content
(prev = curr, zero vectors) at the same sizes: 14 bytes per pixel against the sharpener's 8.  The call is outside the stage timers,
so the HIP events go around every call here: 200 calls after 20 of warm-up.  Every call works on the same buffers again, so they
are served from the 256 MiB Infinity Cache wholly (1080p, 4K) or mostly (8K), as the yardstick's are: the quotient against the
yardstick compares like with like, the shares of 8 TB/s are rates and no HBM figures.  The upscaled frame at strength 16 is timed
twice, at the start and at the end of a size: the difference is the run-to-run spread the other differences are read against.

    python tools/sharpen_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and the kernels' resources (read from the code object's notes), as
profiles/sharpen_4k_profile.txt keeps them.
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

from diff_bench import HBM_PEAK, Events                       # (stage_bench, imported there, puts the repository root on sys.path)
from stage_bench import SIZES, emit, write_json
from linux_fg_amd import capi, synth  # noqa: E402

STRENGTHS = (0, 16, 64)
BYTES_PER_PIXEL = 8


def kernel_resources():
    """{"wide" / "dword": "vgprs ..., sgprs ..., lds ..., scratch ..., waves/SIMD ..."} of the two sharpen kernels, from the notes
    of the library's code objects (llvm-objdump --offloading unbundles them into the working directory, here a temporary one)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(capi.LIB_PATH, d)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=d, capture_output=True, text=True)
        for f in sorted(glob.glob(os.path.join(d, "*gfx950*"))):
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S*sharpen_kernel\S*)", block)
                if not name:
                    continue
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block)[1])  # noqa: E731
                vgprs = get("vgpr_count")
                found["wide" if "ILb1E" in name[1] else "dword"] = (
                    f"vgprs {vgprs}, sgprs {get('sgpr_count')}, lds {get('group_segment_fixed_size')} B, scratch "
                    f"{get('private_segment_fixed_size')} B, waves/SIMD {min(8, 512 // (-(-vgprs // 8) * 8))} by registers")
    return found


def contents(ctx, w, h):
    """(name, a device frame of w x h); the caller destroys the frame."""
    yield "flat", ctx.frame_from(np.full((h, w, 4), 128, np.uint8))
    small, up = ctx.frame_from(synth.make_prev(w // 2, h // 2)), ctx.create_frame(w, h)
    ctx.scale(small, up)
    ctx.sync()
    ctx.destroy_frame(small)
    yield "upscaled synth", up
    yield "noise", ctx.frame_from(np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8))


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
            still = synth.make_prev(w, h)
            p, c, o = ctx.frame_from(still), ctx.frame_from(still), ctx.create_frame(w, h)
            m = ctx.frame_from(np.zeros((h, w, 2), np.int8), capi.FORMAT_MV_S8X2)
            static_us, static_mean = events.per_call_us(ctx, lambda: ctx.interpolate(p, c, m, o, 0.5), a.warmup)
            emit(rows, {"part": "yardstick", "size": size, "call": "lfg_interpolate, static", "median_us": static_us, "mean_us": static_mean,
                        "bytes": 14 * pixels, "share_of_8TBps": 14 * pixels / (static_us * 1e-6) / HBM_PEAK})
            for f in (p, c, m, o):
                ctx.destroy_frame(f)
            out = ctx.create_frame(w, h)
            odd_in, odd_out = ctx.create_frame(w + 1, h), ctx.create_frame(w + 1, h)      # pitches that are no multiple of 16
            repeat = None
            for name, frame in contents(ctx, w, h):
                ctx.copy(frame, capi.Context.wrap(odd_in.data, w, h, pitch=odd_in.pitch))
                paths = (("16-byte", frame, out, w),
                         ("16-byte + remainder", capi.Context.wrap(frame.data, w - 1, h, pitch=frame.pitch), capi.Context.wrap(out.data, w - 1, h, pitch=out.pitch), w - 1),
                         ("dword", capi.Context.wrap(odd_in.data, w, h, pitch=odd_in.pitch), capi.Context.wrap(odd_out.data, w, h, pitch=odd_out.pitch), w))
                for path, src, dst, cols in paths:
                    for strength in STRENGTHS:
                        med, mean = events.per_call_us(ctx, lambda: ctx.sharpen(src, dst, strength), a.warmup)
                        emit(rows, {"part": "sharpen", "size": size, "content": name, "path": path, "strength": strength, "median_us": med,
                                    "mean_us": mean, "bytes": BYTES_PER_PIXEL * cols * h, "share_of_8TBps": BYTES_PER_PIXEL * cols * h / (med * 1e-6) / HBM_PEAK,
                                    "of_static_interpolate": med / static_us, "of_8_14ths": med / (static_us * 8 / 14)})
                if name == "upscaled synth":
                    repeat = frame
                else:
                    ctx.destroy_frame(frame)
            med, mean = events.per_call_us(ctx, lambda: ctx.sharpen(repeat, out, 16), a.warmup)
            emit(rows, {"part": "sharpen, again", "size": size, "content": "upscaled synth", "path": "16-byte", "strength": 16, "median_us": med,
                        "mean_us": mean, "of_static_interpolate": med / static_us})
            for f in (repeat, out, odd_in, odd_out):
                ctx.destroy_frame(f)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/sharpen_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; share_of_8TBps = 8 bytes per pixel (14 for the yardstick) over the median, as a\n"
                    "# share of 8 TB/s; of_static_interpolate = the call's median over lfg_interpolate's on static content, of_8_14ths =\n"
                    "# the same over 8/14 of it (the two calls' bytes).  Every call works on the same buffers again, and they stay in the\n"
                    "# 256 MiB Infinity Cache wholly (1080p, 4K) or mostly (8K), as the yardstick's do: the shares are rates, not HBM\n"
                    "# figures; the quotient compares like with like.\n")
            for kernel, text in sorted(kernel_resources().items()):
                f.write(f"# sharpen_kernel<{kernel}>: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
