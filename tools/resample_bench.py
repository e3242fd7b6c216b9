"""Time lfg_resample: every filter at 1080p -> 4K, 1080p -> 1440p, 4K -> 1080p and 4K -> 720p on a `synth` frame, and in the same
run, as the yardstick, lfg_scale on the same frames -- the parent's own kernels: the generic one everywhere, and at 1080p -> 4K
both the 2x kernel and the generic one (an output pitch that is no multiple of 16 selects it; lfg_scale_last_kernel says which
ran).  HIP events go around every call: 200 calls after 20 of warm-up.  Every call works on the same buffers again, so they are
served from the 256 MiB Infinity Cache: the shares of 8 TB/s are rates and no HBM figures, and the quotient against the yardstick
compares like with like.  Lanczos-3 is timed twice per size pair, first and last: the difference is the run-to-run spread.

    python tools/resample_bench.py [--calls 200] [--warmup 20] [--json out.json] [--out profile.txt]
    python tools/resample_bench.py --drive '1080p->4k:lanczos3' --calls 50      the calls alone, for a profiler

--out writes the rows, stamped with the library's sha and the kernel's resources (read from the code object's notes), as
profiles/resample_4k_profile.txt keeps them.
"""
from __future__ import annotations

import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import tempfile

from diff_bench import HBM_PEAK, Events                       # (stage_bench, imported there, puts the repository root on sys.path)
from stage_bench import emit, write_json
from linux_fg_amd import capi, synth  # noqa: E402

PAIRS = (("1080p->4k", (1920, 1080), (3840, 2160)), ("1080p->1440p", (1920, 1080), (2560, 1440)),
         ("4k->1080p", (3840, 2160), (1920, 1080)), ("4k->720p", (3840, 2160), (1280, 720)))
FILTERS = (("nearest", capi.FILTER_NEAREST), ("bilinear", capi.FILTER_BILINEAR), ("catmull-rom", capi.FILTER_CATMULL_ROM),
           ("mitchell", capi.FILTER_MITCHELL), ("lanczos2", capi.FILTER_LANCZOS2), ("lanczos3", capi.FILTER_LANCZOS3))
SCALE_KERNELS = {0: "scale_generic_kernel", 1: "scale_2x_kernel"}


def kernel_resources(kernel="resample_kernel"):
    """"vgprs ..., sgprs ..., lds ..., scratch ..., waves/SIMD ..." of `kernel`, from the notes of the library's code
    objects (llvm-objdump --offloading unbundles them into the working directory, here a temporary one)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(capi.LIB_PATH, d)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=d, capture_output=True, text=True)
        for f in sorted(glob.glob(os.path.join(d, "*gfx950*"))):
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                if not re.search(rf"\.name:\s+\S*{kernel}\S*", block):
                    continue
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block)[1])  # noqa: E731
                vgprs = get("vgpr_count")
                return (f"vgprs {vgprs}, sgprs {get('sgpr_count')}, lds {get('group_segment_fixed_size')} B static + 512 B per source row of a "
                        f"tile (at most 32 KiB), scratch {get('private_segment_fixed_size')} B, waves/SIMD {min(8, 512 // (-(-vgprs // 8) * 8))} by registers")
    return "not found"


def drive(what, calls):
    """`calls` calls of lfg_resample for PAIR:FILTER (e.g. 1080p->4k:lanczos3) and nothing else: what a profiler is put around."""
    pair, name = what.split(":")
    (w, h), (ow, oh) = next((i, o) for p, i, o in PAIRS if p == pair)
    with capi.Context(0) as ctx:
        src, dst = ctx.frame_from(synth.make_prev(w, h)), ctx.create_frame(ow, oh)
        for _ in range(calls):
            ctx.resample(src, dst, dict(FILTERS)[name])
        ctx.sync()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--drive", default=None, metavar="PAIR:FILTER", help="only enqueue --calls calls of one pair and filter, for a profiler")
    a = ap.parse_args()
    if a.drive:
        return drive(a.drive, a.calls)
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        for pair, (w, h), (ow, oh) in PAIRS:
            nbytes = 4 * (w * h + ow * oh)
            host = synth.make_prev(w, h)
            src, dst = ctx.frame_from(host), ctx.create_frame(ow, oh)
            odd = ctx.create_frame(ow + 1, oh)                             # an output pitch that is no multiple of 16
            odd_dst = capi.Context.wrap(odd.data, ow, oh, pitch=odd.pitch)
            yard = {}
            for name, frame in (("tight", dst), ("odd pitch", odd_dst)):
                med, mean = events.per_call_us(ctx, lambda: ctx.scale(src, frame), a.warmup)
                kernel = SCALE_KERNELS.get(ctx.lib.lfg_scale_last_kernel(ctx.h), "?")
                yard[kernel] = med
                emit(rows, {"part": "yardstick", "pair": pair, "call": "lfg_scale", "output": name, "kernel": kernel, "median_us": med, "mean_us": mean,
                            "bytes": nbytes, "share_of_8TBps": nbytes / (med * 1e-6) / HBM_PEAK})
            for name, filt in (FILTERS[-1],) + FILTERS:
                med, mean = events.per_call_us(ctx, lambda: ctx.resample(src, dst, filt), a.warmup)
                row = {"part": "resample", "pair": pair, "filter": name, "median_us": med, "mean_us": mean, "bytes": nbytes,
                       "share_of_8TBps": nbytes / (med * 1e-6) / HBM_PEAK}
                for kernel, us in yard.items():
                    row["of_" + kernel] = med / us
                emit(rows, row)
            for f in (src, dst, odd):
                ctx.destroy_frame(f)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/resample_bench.py --calls {a.calls} --warmup {a.warmup}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; share_of_8TBps = 4 bytes per input and per output pixel over the median, as a share\n"
                    "# of 8 TB/s; of_<kernel> = the call's median over lfg_scale's through that kernel on the same frames.  Every call\n"
                    "# works on the same buffers again, and they stay in the 256 MiB Infinity Cache: the shares are rates, not HBM\n"
                    "# figures; the quotient compares like with like.  Lanczos-3 comes first and last: the run-to-run spread.\n")
            f.write(f"# resample_kernel: {kernel_resources()}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
