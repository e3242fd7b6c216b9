"""Time lfg_resample_antiring: Lanczos-3 and Catmull-Rom at strength 64, 1080p -> 4K and 1080p -> 1440p, on a `synth` frame, and in
the same run, as the yardstick, lfg_resample under the same filter on the same frames -- never a stored number.  HIP events go
around every call: 200 calls after 20 of warm-up, medians.  Each pair of sizes times the yardstick before and after the
anti-ringed call: the two medians show the run-to-run spread next to the quotient.  Every call works on the same buffers again,
so they are served from the 256 MiB Infinity Cache: rates, no HBM figures; the quotient compares like with like.

    python tools/antiring_bench.py [--calls 200] [--warmup 20] [--strength 64] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and both kernels' resources (read from the code object's notes), as
profiles/antiring_4k_profile.txt keeps them.
"""
from __future__ import annotations

import hashlib
import json

from diff_bench import HBM_PEAK, Events                       # (stage_bench, imported there, puts the repository root on sys.path)
from resample_bench import kernel_resources
from stage_bench import emit, write_json
from linux_fg_amd import capi, synth  # noqa: E402

PAIRS = (("1080p->4k", (1920, 1080), (3840, 2160)), ("1080p->1440p", (1920, 1080), (2560, 1440)))
FILTERS = (("lanczos3", capi.FILTER_LANCZOS3), ("catmull-rom", capi.FILTER_CATMULL_ROM))


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--strength", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        for pair, (w, h), (ow, oh) in PAIRS:
            nbytes = 4 * (w * h + ow * oh)
            src, dst = ctx.frame_from(synth.make_prev(w, h)), ctx.create_frame(ow, oh)
            for name, filt in FILTERS:
                before, _ = events.per_call_us(ctx, lambda: ctx.resample(src, dst, filt), a.warmup)
                med, mean = events.per_call_us(ctx, lambda: ctx.resample_antiring(src, dst, filt, a.strength), a.warmup)
                after, _ = events.per_call_us(ctx, lambda: ctx.resample(src, dst, filt), a.warmup)
                plain = (before + after) / 2
                emit(rows, {"pair": pair, "filter": name, "strength": a.strength, "antiring_median_us": med, "antiring_mean_us": mean,
                            "resample_median_us_before": before, "resample_median_us_after": after, "of_resample": med / plain, "bytes": nbytes,
                            "share_of_8TBps": nbytes / (med * 1e-6) / HBM_PEAK})
            ctx.destroy_frame(src)
            ctx.destroy_frame(dst)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/antiring_bench.py --calls {a.calls} --warmup {a.warmup} --strength {a.strength}: HIP events around every call,\n"
                    f"# {a.calls} calls after {a.warmup} of warm-up, medians in us.  of_resample = lfg_resample_antiring's median over the mean of\n"
                    "# lfg_resample's two medians of the same run (same filter, same frames; taken before and after: their distance is the\n"
                    "# spread).  share_of_8TBps = 4 bytes per input and per output pixel over the median, as a share of 8 TB/s: the buffers\n"
                    "# stay in the 256 MiB Infinity Cache, so a rate and no HBM figure.\n")
            f.write(f"# resample_antiring_kernel: {kernel_resources('resample_antiring_kernel')}\n")
            f.write(f"# resample_kernel: {kernel_resources()}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
