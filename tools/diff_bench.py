"""Time the frame comparison: lfg_frame_diff at 1080p, 4K and 8K on five contents -- identical frames, b = a +- 1 on random
channels, an upscale (half size -> size, lfg_scale) against itself shifted by one pixel, unrelated frames, 0 against 255 --
through both load paths (16-byte: frames as lfg_frame_create makes them; dword: the same pixels in frames one pixel wider,
whose pitch is no multiple of 16) and with accumulate 0 and 1.  In the same run, as the yardstick, lfg_interpolate on static
content (prev = curr, zero vectors) at the same sizes: 10 bytes read and 4 written per pixel against the comparison's 8 read.
lfg_frame_diff is outside the stage timers, so the HIP events go around every call here: 200 calls after 20 of warm-up.

    python tools/diff_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and the kernel's resources (read from the code object's notes), as
profiles/diff_4k_profile.txt keeps them.
"""
from __future__ import annotations

import ctypes
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

from stage_bench import SIZES, emit, write_json                # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402

HBM_PEAK = 8.0e12                                              # bytes per second, the chip's specification
_hip = ctypes.CDLL("libamdhip64.so")
_hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
_hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
_hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
_hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]


def hip(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


class Events:
    """`calls` pairs of HIP events on the context's stream."""

    def __init__(self, ctx, calls):
        self.stream = ctx.lib.lfg_context_get_stream(ctx.h)
        self.pairs = []
        for _ in range(calls):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            hip(_hip.hipEventCreate(ctypes.byref(a)))
            hip(_hip.hipEventCreate(ctypes.byref(b)))
            self.pairs.append((a, b))

    def per_call_us(self, ctx, fn, warmup):
        """Microseconds per call of fn() between its two events: (median, mean) over the calls."""
        for _ in range(warmup):
            fn()
        ctx.sync()
        for a, b in self.pairs:
            hip(_hip.hipEventRecord(a, self.stream))
            fn()
            hip(_hip.hipEventRecord(b, self.stream))
        hip(_hip.hipEventSynchronize(self.pairs[-1][1]))
        us = []
        for a, b in self.pairs:
            ms = ctypes.c_float()
            hip(_hip.hipEventElapsedTime(ctypes.byref(ms), a, b))
            us.append(1000.0 * ms.value)
        return float(np.median(us)), float(np.mean(us))


def contents(ctx, w, h):
    """(name, a, b) as host arrays."""
    a = synth.make_prev(w, h)
    yield "identical", a, a
    rng = np.random.default_rng(3)
    step = np.zeros((h, w, 4), np.int16)
    np.put_along_axis(step, rng.integers(0, 4, (h, w, 1)), rng.choice([-1, 1], size=(h, w, 1)).astype(np.int16), axis=-1)
    yield "+-1", a, np.clip(a.astype(np.int16) + step, 0, 255).astype(np.uint8)
    small, big = ctx.frame_from(synth.make_prev(w // 2, h // 2)), ctx.create_frame(w, h)
    ctx.scale(small, big)
    up = ctx.download(big)
    ctx.destroy_frame(small)
    ctx.destroy_frame(big)
    yield "upscale-shifted-1px", up, np.roll(up, 1, axis=1)
    yield "unrelated", rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yield "0-against-255", np.zeros((h, w, 4), np.uint8), np.full((h, w, 4), 255, np.uint8)


def padded(ctx, host):
    """`host` in a frame one pixel wider: a pitch that is no multiple of 16 for every size here.  (the frame, the view)"""
    h, w = host.shape[:2]
    big = ctx.create_frame(w + 1, h)
    ctx.upload(big, np.concatenate([host, np.zeros((h, 1, 4), np.uint8)], axis=1))
    return big, capi.Context.wrap(big.data, w, h, pitch=(w + 1) * 4)


def kernel_resources(kernel="frame_diff_kernel"):
    """{"wide" / "dword": "vgprs ..., lds ..., waves/SIMD ..."} of the two variants of `kernel`, from the notes of the library's
    code objects (llvm-objdump --offloading unbundles them into the working directory, here a temporary one)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(capi.LIB_PATH, d)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=d, capture_output=True, text=True)
        for f in sorted(glob.glob(os.path.join(d, "*gfx950*"))):
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(rf"\.name:\s+(\S*{kernel}\S*)", block)
                if not name:
                    continue
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block)[1])  # noqa: E731
                vgprs = get("vgpr_count")
                found["wide" if "ILb1E" in name[1] else "dword"] = (
                    f"vgprs {vgprs}, sgprs {get('sgpr_count')}, lds {get('group_segment_fixed_size')} B, scratch "
                    f"{get('private_segment_fixed_size')} B, waves/SIMD {min(8, 512 // (-(-vgprs // 8) * 8))} by registers")
    return found


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
            # the yardstick: lfg_interpolate on static content
            still = synth.make_prev(w, h)
            p, c, o = ctx.frame_from(still), ctx.frame_from(still), ctx.create_frame(w, h)
            m = ctx.frame_from(np.zeros((h, w, 2), np.int8), capi.FORMAT_MV_S8X2)
            static_us, static_mean = events.per_call_us(ctx, lambda: ctx.interpolate(p, c, m, o, 0.5), a.warmup)
            emit(rows, {"part": "yardstick", "size": size, "call": "lfg_interpolate, static", "median_us": static_us, "mean_us": static_mean,
                        "bytes": 14 * pixels, "share_of_8TBps": 14 * pixels / (static_us * 1e-6) / HBM_PEAK})
            for f in (p, c, m, o):
                ctx.destroy_frame(f)
            r = ctx.create_diff_record()
            for name, x, y in contents(ctx, w, h):
                fx, fy = ctx.frame_from(x), ctx.frame_from(y)
                bx, vx = padded(ctx, x)
                by, vy = padded(ctx, y)
                for path, (fa, fb) in (("16-byte", (fx, fy)), ("dword", (vx, vy))):
                    ctx.frame_diff(fa, fb, r)
                    record = ctx.read_diff_record(r)
                    s = capi.summarize(record)
                    row = {"part": "frame_diff", "size": size, "content": name, "loads": path, "differing": s["differing"],
                           "max_abs": s["max_abs"], "bins": sum(1 for v in record[2] if v)}
                    for label, acc in (("write", False), ("accumulate", True)):
                        med, mean = events.per_call_us(ctx, lambda: ctx.frame_diff(fa, fb, r, 0xF, acc), a.warmup)
                        row[f"{label}_median_us"], row[f"{label}_mean_us"] = med, mean
                    row["share_of_8TBps"] = 8 * pixels / (row["write_median_us"] * 1e-6) / HBM_PEAK
                    row["of_static_interpolate"] = row["write_median_us"] / static_us
                    emit(rows, row)
                for f in (fx, fy, bx, by):
                    ctx.destroy_frame(f)
            ctx.destroy_frame(r)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/diff_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; share_of_8TBps = 8 bytes per pixel (14 for the yardstick) over the median, as a\n"
                    "# share of 8 TB/s; of_static_interpolate = the comparison's median over lfg_interpolate's on static content.\n")
            for kernel, text in kernel_resources().items():
                f.write(f"# frame_diff_kernel<{kernel}>: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
