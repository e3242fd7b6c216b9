"""Time static-overlay protection: lfg_interpolate_compensated_masked beside lfg_interpolate_compensated on the same inputs in the
same run, with one factor and with three (t = 1/4, 1/2, 3/4), and lfg_static_mask alone, at 1080p, 4K and 8K on four contents: a
pan, the pan with 1 % of its pixels static (a HUD of scattered 16 x 16 tiles), a still (every pixel static) and uncorrelated
frames.  The vectors come from lfg_motion under the intended semantics; the mask is lfg_static_mask's at tolerance 0.  The mask
call is outside the stage timers, so the HIP events go around every call here: 200 calls after 20 of warm-up.  No target is
fixed; the yardstick is the unmasked call of the same run.

    python tools/overlay_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and the kernels' resources (read from the code object's notes), as
profiles/overlay_4k_profile.txt keeps them.
"""
from __future__ import annotations

import argparse
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
from linux_fg_amd import capi, synth  # noqa: E402

FACTORS = [0.25, 0.5, 0.75]
KERNELS = "mc_project_kernel|mc_interpolate_kernel|mc_project_masked_kernel|mc_interpolate_masked_kernel|static_mask_kernelILb[01]E"


def kernel_resources(kernels=KERNELS):
    """{kernel: "vgprs ..., sgprs ..., lds ..., scratch ..., waves/SIMD ..."} of the kernels named by the pattern `kernels` (default:
    the unmasked and the masked kernels and the mask kernel's two instances), from the notes of the library's code objects."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        lib = shutil.copy(capi.LIB_PATH, d)
        subprocess.run([f"{llvm}/llvm-objdump", "--offloading", lib], cwd=d, capture_output=True, text=True)
        for f in sorted(glob.glob(os.path.join(d, "*gfx950*"))):
            notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", f], capture_output=True, text=True).stdout
            for block in notes.split("  - .agpr_count:")[1:]:
                name = re.search(rf"\.name:\s+\S*?\d\d({kernels})E", block)
                if not name:
                    continue
                get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block)[1])  # noqa: E731
                vgprs = get("vgpr_count")
                label = name[1].replace("ILb1E", "<16-byte loads>").replace("ILb0E", "<dword loads>")
                found[label] = (f"vgprs {vgprs}, sgprs {get('sgpr_count')}, lds {get('group_segment_fixed_size')} B, scratch "
                                f"{get('private_segment_fixed_size')} B, waves/SIMD {min(8, 512 // (-(-vgprs // 8) * 8))} by registers")
    return found


def contents(w, h):
    """(name, prev, curr)"""
    prev = synth.make_prev(w, h)
    pan = synth.translate(prev, (6, -4))
    yield "pan(6,-4)", prev, pan
    hud_prev, hud_curr = prev.copy(), pan.copy()             # 1 % of the pixels: 16 x 16 tiles of one noise image, at the same places
    rng = np.random.default_rng(11)
    tiles = w * h // 100 // 256
    noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for x, y in zip(rng.integers(0, w // 16, tiles) * 16, rng.integers(0, h // 16, tiles) * 16):
        hud_prev[y:y + 16, x:x + 16] = hud_curr[y:y + 16, x:x + 16] = noise[y:y + 16, x:x + 16]
    yield "pan+1%static", hud_prev, hud_curr
    yield "still", prev, prev.copy()
    a, b = synth.make_uncorrelated_pair(w, h)
    yield "uncorrelated", a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k,8k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        events = Events(ctx, a.calls)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                ctx.motion(p, c, m)
                owner, mask = ctx.create_mask(w, h)
                ctx.static_mask(p, c, mask, 0)
                static = int((ctx.download_mask(owner, mask)[0] != 0).sum())
                outs = [ctx.create_frame(w, h) for _ in FACTORS]
                r = {"size": size, "content": name, "static_permille": round(1000.0 * static / (w * h), 2)}
                calls = (("mask_us", lambda: ctx.static_mask(p, c, mask, 0)),
                         ("plain_us", lambda: ctx.interpolate_compensated(p, c, m, outs[0], 0.5, 48)),
                         ("masked_us", lambda: ctx.interpolate_compensated_masked(p, c, m, mask, outs[0], 0.5, 48)),
                         ("plain_x3_us", lambda: ctx.interpolate_compensated_multi(p, c, m, outs, FACTORS, 48)),
                         ("masked_x3_us", lambda: ctx.interpolate_compensated_masked_multi(p, c, m, mask, outs, FACTORS, 48)))
                for key, fn in calls:
                    r[key] = round(events.per_call_us(ctx, fn, a.warmup)[0], 2)              # the median
                r["masked_over_plain"] = round(r["masked_us"] / r["plain_us"], 3)
                r["masked_x3_over_plain_x3"] = round(r["masked_x3_us"] / r["plain_x3_us"], 3)
                r["extra_over_mask_kernel"] = round((r["masked_us"] - r["plain_us"]) / r["mask_us"], 3)
                emit(rows, r)
                for f in [p, c, m, owner] + outs:
                    ctx.destroy_frame(f)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/overlay_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                    "# warm-up, medians in us.  plain = lfg_interpolate_compensated[_multi], masked = lfg_interpolate_compensated_masked[_multi]\n"
                    "# on the same inputs with lfg_static_mask's mask at tolerance 0, mask = lfg_static_mask alone; x3 = the factors 1/4, 1/2,\n"
                    "# 3/4.  extra_over_mask_kernel = (masked - plain) / mask.  Every call works on the same buffers again: at 1080p and 4K\n"
                    "# they stay in the 256 MiB Infinity Cache, so the quotients compare like with like and are no HBM figures.\n")
            for kernel, text in sorted(kernel_resources().items()):
                f.write(f"# {kernel}: {text}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
