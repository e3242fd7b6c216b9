"""Time lfg_resample_light under Lanczos-3: both modes at 1080p -> 4K and 1080p -> 1440p, linear light alone at 4K -> 1080p and
1080p -> 640 x 360 (the sigmoid is refused where an axis shrinks), and in the same run, as the yardstick, lfg_resample under the
same filter on the same frames -- never a stored number.  HIP events go around every call: 200 calls after 20 of warm-up,
medians.  Each shape times the yardstick before and after the calls in light: the two medians show the run-to-run spread next to
the quotients.  Two contents, a `synth` frame and random bytes: the kernel has no branch on the content, but its table lookups
in LDS conflict where neighbouring lanes read unrelated bytes and broadcast where they read the same.  Every call works on the
same buffers again, so they are served from the 256 MiB Infinity Cache: rates, no HBM figures; the quotient compares like with
like.

    python tools/light_bench.py [--calls 200] [--warmup 20] [--json out.json] [--out profile.txt]

--out writes the rows, stamped with the library's sha and both kernels' resources (read from the code object's notes), as
profiles/light_4k_profile.txt keeps them.
"""
from __future__ import annotations

import hashlib
import json

import numpy as np

from diff_bench import HBM_PEAK, Events                       # (stage_bench, imported there, puts the repository root on sys.path)
from resample_bench import kernel_resources
from stage_bench import emit, write_json
from linux_fg_amd import capi, synth  # noqa: E402

PAIRS = (("1080p->4k", (1920, 1080), (3840, 2160)), ("1080p->1440p", (1920, 1080), (2560, 1440)),
         ("4k->1080p", (3840, 2160), (1920, 1080)), ("1080p->360p", (1920, 1080), (640, 360)))
MODES = (("linear", capi.LIGHT_LINEAR), ("sigmoid", capi.LIGHT_SIGMOID))
CONTENTS = (("synth", lambda w, h: synth.make_prev(w, h)),
            ("random bytes", lambda w, h: np.random.default_rng(1).integers(0, 256, (h, w, 4)).astype(np.uint8)))


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    filt = capi.FILTER_LANCZOS3
    rows = []
    with capi.Context(0) as ctx:
        events = Events(ctx, a.calls)
        for pair, (w, h), (ow, oh) in PAIRS:
            nbytes = 4 * (w * h + ow * oh)
            dst = ctx.create_frame(ow, oh)
            for content, make in CONTENTS:
                src = ctx.frame_from(make(w, h))
                before, _ = events.per_call_us(ctx, lambda: ctx.resample(src, dst, filt), a.warmup)
                timed = {}
                for name, mode in MODES:
                    if mode == capi.LIGHT_SIGMOID and (ow < w or oh < h):
                        continue
                    timed[name] = events.per_call_us(ctx, lambda: ctx.resample_light(src, dst, filt, mode), a.warmup)[0]
                after, _ = events.per_call_us(ctx, lambda: ctx.resample(src, dst, filt), a.warmup)
                plain = (before + after) / 2
                row = {"pair": pair, "filter": "lanczos3", "content": content, "resample_median_us_before": before, "resample_median_us_after": after,
                       "bytes": nbytes}
                for name, med in timed.items():
                    row.update({f"{name}_median_us": med, f"{name}_of_resample": med / plain, f"{name}_share_of_8TBps": nbytes / (med * 1e-6) / HBM_PEAK})
                emit(rows, row)
                ctx.destroy_frame(src)
            ctx.destroy_frame(dst)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/light_bench.py --calls {a.calls} --warmup {a.warmup}: HIP events around every call, {a.calls} calls after\n"
                    f"# {a.warmup} of warm-up, medians in us, Lanczos-3.  *_of_resample = lfg_resample_light's median in that mode over the mean of\n"
                    "# lfg_resample's two medians of the same run (same filter, same frames; taken before and after: their distance is the\n"
                    "# spread).  *_share_of_8TBps = 4 bytes per input and per output pixel over the median, as a share of 8 TB/s: the buffers\n"
                    "# stay in the 256 MiB Infinity Cache, so a rate and no HBM figure.  No sigmoid where an axis shrinks: it is refused.\n")
            f.write(f"# resample_light_kernel: {kernel_resources('resample_light_kernel')} (+ 1024 B of tables)\n")
            f.write(f"# resample_kernel: {kernel_resources()}\n")
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
