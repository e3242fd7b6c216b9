"""Time the colour conversion: lfg_nv12_to_rgba and lfg_rgba_to_nv12 at 1080p, 4K and 8K under both chroma sitings (BT.709,
limited range; matrix and range only change the numbers in the kernel's arguments), through the 8 x 2 items (planes and frames
as lfg_frame_create makes them) and, at 4K, through the one-quad items as well (the same bytes at pitches that allow no aligned
access).  In the same run, as the yardstick, lfg_interpolate on static content (prev = curr, zero vectors) at the same sizes:
14 bytes per pixel against a conversion's 5.5.  The conversions are outside the stage timers, so the HIP events go around every
call here: 200 calls after 20 of warm-up.  Every call converts the same buffers again, so they are served from the 256 MiB
Infinity Cache wholly (1080p, 4K) or mostly (8K), as the yardstick's are: the quotient against the yardstick compares like with
like, the shares of 8 TB/s are rates and no HBM figures.

    python tools/convert_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and the kernels' resources (read from the code object's notes), as
profiles/convert_4k_profile.txt keeps them.
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

SITINGS = (("replicate", capi.CHROMA_REPLICATE), ("left", capi.CHROMA_LEFT))
BYTES_PER_PIXEL = 5.5


def kernel_resources():
    """{kernel: "vgprs ..., sgprs ..., lds ..., scratch ..., waves/SIMD ..."} of the four conversion kernels, from the notes of the
    library's code objects (llvm-objdump --offloading unbundles them into the working directory, here a temporary one)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(capi.LIB_PATH, d)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=d, capture_output=True, text=True)
        for f in sorted(glob.glob(os.path.join(d, "*gfx950*"))):
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+\S*?(nv12_to_rgba_kernel|rgba_to_nv12_kernel)ILi(\d)E", block)
                if not name:
                    continue
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block)[1])  # noqa: E731
                vgprs = get("vgpr_count")
                found[f"{name[1]}<{'left' if name[2] == '1' else 'replicate'}>"] = (
                    f"vgprs {vgprs}, sgprs {get('sgpr_count')}, lds {get('group_segment_fixed_size')} B, scratch "
                    f"{get('private_segment_fixed_size')} B, waves/SIMD {min(8, 512 // (-(-vgprs // 8) * 8))} by registers")
    return found


def pitched_nv12(ctx, w, h, pad):
    """NV12 planes `pad` bytes wider than the image: (the frame that owns them, the lfg_nv12)."""
    f = ctx.create_frame((w + pad) // 2, h * 3 // 2, capi.FORMAT_MV_S8X2)
    return f, capi.Nv12(f.data, f.data + (w + pad) * h, w, h, w + pad, w + pad)


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
            for f in (c, m, o):
                ctx.destroy_frame(f)
            layouts = [("8x2", ctx.create_nv12(w, h), ctx.create_frame(w, h))]
            if size == "4k":                                   # 2 bytes (NV12) and 1 pixel (RGBA) of padding: nothing is aligned
                padded = ctx.create_frame(w + 1, h)
                layouts.append(("quad", pitched_nv12(ctx, w, h, 2), padded))
            for items, (owner, planes), frame in layouts:
                rgba = capi.Context.wrap(frame.data, w, h, pitch=frame.pitch)
                for name, siting in SITINGS:
                    ctx.rgba_to_nv12(capi.Context.wrap(p.data, w, h), planes, capi.YUV_BT709, capi.YUV_LIMITED, siting)   # content
                    for call, fn in (("lfg_nv12_to_rgba", lambda: ctx.nv12_to_rgba(planes, rgba, capi.YUV_BT709, capi.YUV_LIMITED, siting)),
                                     ("lfg_rgba_to_nv12", lambda: ctx.rgba_to_nv12(rgba, planes, capi.YUV_BT709, capi.YUV_LIMITED, siting))):
                        med, mean = events.per_call_us(ctx, fn, a.warmup)
                        emit(rows, {"part": "convert", "size": size, "call": call, "siting": name, "items": items, "median_us": med,
                                    "mean_us": mean, "bytes": int(BYTES_PER_PIXEL * pixels),
                                    "share_of_8TBps": BYTES_PER_PIXEL * pixels / (med * 1e-6) / HBM_PEAK, "of_static_interpolate": med / static_us})
                ctx.destroy_frame(owner)
                ctx.destroy_frame(frame)
            ctx.destroy_frame(p)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/convert_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, median and mean in us; share_of_8TBps = 5.5 bytes per pixel (14 for the yardstick) over the median, as a\n"
                    "# share of 8 TB/s; of_static_interpolate = the conversion's median over lfg_interpolate's on static content.\n"
                    "# Every call converts the same buffers again, and they stay in the 256 MiB Infinity Cache wholly (1080p, 4K) or mostly\n"
                    "# (8K), as the yardstick's do: the shares are rates, not HBM figures; the quotient compares like with like.\n")
            for kernel, text in sorted(kernel_resources().items()):
                f.write(f"# {kernel}: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
