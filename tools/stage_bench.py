"""What the stage timers (pyramid_bench.py, compensated_bench.py, refine_bench.py) share: the frame sizes, the arguments, the
device-event timing loop (lfg_profile_*: HIP events around every stage launch) and the output rows."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160), "8k": (7680, 4320)}


def arguments(sizes):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default=sizes)
    ap.add_argument("--json", default=None)
    return ap.parse_args()


def per_call_ms(ctx, fn, calls, warmup, *stages):
    """Milliseconds per call of fn() on the device, summed over `stages`, after `warmup` calls that are not timed."""
    for _ in range(warmup):
        fn()
    ctx.sync()
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(calls):
        fn()
    ms = [ctx.profile_get(s)[0] for s in stages]
    ctx.profile_enable(False)
    return sum(ms) / calls


def emit(rows, row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def write_json(path, rows):
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)
