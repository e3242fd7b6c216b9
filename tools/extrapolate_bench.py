"""Time lfg_extrapolate_compensated beside lfg_interpolate_compensated on the same inputs in the same run, at 1080p, 4K and 8K on
the five contents of tools/compensated_bench.py.  HIP events around every call, 200 calls after 20 of warm-up; the vectors come
from lfg_motion under the intended semantics, except for the dense random field.  No duration is fixed in advance: the stage
does less than the compensated interpolation (one gathered fetch instead of two, the same clear and projection), so the bar is
the compensated call of the same run.  That call is timed twice, before and after the extrapolation; the distance between its
two medians is the run's own spread, and the only margin the comparison gets.

    python tools/extrapolate_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k,8k] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and the kernels' resources (read from the code object's notes), as
profiles/extrapolate_4k_profile.txt keeps them.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys

import overlay_bench                                          # (its imports put the repository root on sys.path)
from compensated_bench import contents
from diff_bench import Events
from stage_bench import SIZES, emit, write_json
from linux_fg_amd import capi  # noqa: E402

OUT = "profiles/extrapolate_4k_profile.txt"
KERNELS = "mc_project_kernel|mc_interpolate_kernel|ex_project_kernel|ex_sample_kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="1080p,4k,8k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        events = Events(ctx, a.calls)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr, vectors, ms in contents(w, h):
                p, c = ctx.frame_from(prev), ctx.frame_from(curr)
                if vectors is None:
                    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
                    ctx.motion(p, c, m)
                else:
                    m = ctx.frame_from(vectors, capi.FORMAT_MV_S8X2)
                o = ctx.create_frame(w, h)
                r = {"size": size, "content": name, "match_sad": ms}
                compensated = lambda: ctx.interpolate_compensated(p, c, m, o, 0.5, ms)  # noqa: E731
                r["compensated_us"] = round(events.per_call_us(ctx, compensated, a.warmup)[0], 2)             # medians
                r["extrapolate_a0.5_us"] = round(events.per_call_us(ctx, lambda: ctx.extrapolate_compensated(p, c, m, o, 0.5, ms), a.warmup)[0], 2)
                r["extrapolate_a1_us"] = round(events.per_call_us(ctx, lambda: ctx.extrapolate_compensated(p, c, m, o, 1.0, ms), a.warmup)[0], 2)
                r["compensated_again_us"] = round(events.per_call_us(ctx, compensated, a.warmup)[0], 2)
                r["spread_us"] = round(abs(r["compensated_us"] - r["compensated_again_us"]), 2)
                bar = max(r["compensated_us"], r["compensated_again_us"])
                r["slower_than_compensated"] = max(r["extrapolate_a0.5_us"], r["extrapolate_a1_us"]) > bar
                emit(rows, r)
                for f in (p, c, m, o):
                    ctx.destroy_frame(f)
    write_json(a.json, rows)
    with open(a.out, "w") as f:
        f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
        f.write(f"# python tools/extrapolate_bench.py {' '.join(sys.argv[1:])}: HIP events around every call, {a.calls} calls after {a.warmup} of\n"
                "# warm-up, medians in us.  compensated = lfg_interpolate_compensated at t = 0.5, timed before and after the two\n"
                "# lfg_extrapolate_compensated columns (a = 0.5, a = 1) on the same inputs; spread = the distance between its two medians;\n"
                "# slower_than_compensated: an extrapolation median above both.  Every call works on the same buffers again: at 1080p and\n"
                "# 4K they stay in the 256 MiB Infinity Cache, so the columns compare like with like and are no HBM figures.\n")
        for kernel, text in sorted(overlay_bench.kernel_resources(KERNELS).items()):
            f.write(f"# {kernel}: {text}\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
