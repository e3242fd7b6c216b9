"""Time the fill plane (lfg_set_hole_reach, lfg_hole_fill_plane) next to the 16-pixel hole walk it replaces.  HIP events around
every call (torch events on the stream the context is given), medians with the 10th and 90th percentile as the run's spread.

    python tools/fill_bench.py [--calls 200] [--warmup 20] [--sizes 1080p,4k] [--json out.json]

Rows, per size:
  calls    lfg_interpolate_compensated at t = 0.5 on four contents with the setting off -- the unchanged call, the yardstick of
           the run -- and at reach 16, 64 and 255;
  growth   lfg_hole_fill_plane alone on a key image that is all holes but for donors on the frame's border, at reach 16 and 255;
  quality  wrong pixels (tests/fill_model.py: wrong_pixels) of lfg_interpolate_frames with the pyramid and the compensated
           interpolator against the true middle frame, on scenes B and A of DESIGN.md section 4.19 with frame, square and
           position scaled to 1920 x 1080 and the motion kept, setting off and reach 16, 32, 64, 255;
  band     the same call at reach 255 and 16 with the column pass's band height set through LFG_FILL_BAND (a context reads it
           when it is made), for the choice of kFillBand.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from stage_bench import SIZES, arguments, emit, write_json      # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402
from tests import fill_model  # noqa: E402      (the scene of DESIGN.md section 4.19 and its count of wrong pixels)

REACHES = (-1, 16, 64, 255)
BANDS = (16, 32, 64, 128, 256)
MV = capi.FORMAT_MV_S8X2


def contents(w, h):
    """(name, prev, curr, vectors or None for lfg_motion's)"""
    prev = synth.make_prev(w, h)
    pan = synth.translate(prev, (6, -4))
    yield "pan(6,-4)", prev, pan, None
    objects = pan.copy()                                    # two 256 x 256 blocks of prev moved by their own vectors over the pan
    for (x, y), (dx, dy) in (((w // 4, h // 4), (12, 0)), ((w // 2, h // 2), (-10, 8))):
        objects[y + dy:y + dy + 256, x + dx:x + dx + 256] = prev[y:y + 256, x:x + 256]
    yield "objects over pan", prev, objects, None
    a, b = synth.make_uncorrelated_pair(w, h)
    yield "uncorrelated", a, b, None
    # the kind of scene the reach is for: a noise square of a quarter of the height moves by (120, 0) over a pan of (4, 2); true field
    (fast_prev, fast_curr), field = fill_model.fast_scene(w, h, h // 4, (w // 8, h // 8), (4, 2), (120, 0), frames=(0.0, 1.0))
    yield "fast object", fast_prev, fast_curr, field


def border_donors(w, h):
    K = np.full((h, w), 0xFFFFFFFF, np.uint32)
    K[0, :] = K[-1, :] = K[:, 0] = K[:, -1] = (65535 - 25) << 16 | (128 + 4) << 8 | (128 + 3)
    return K.view(np.uint8).reshape(h, w, 4)


class Timer:
    def __init__(self, ctx, stream, calls, warmup):
        self.ctx, self.stream, self.calls, self.warmup = ctx, stream, calls, warmup

    def __call__(self, fn):
        """(median, 10th percentile, 90th percentile) of fn()'s device time in microseconds."""
        for _ in range(self.warmup):
            fn()
        self.ctx.sync()
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(self.calls)]
        for begin, end in events:
            begin.record(self.stream)
            fn()
            end.record(self.stream)
        self.stream.synchronize()
        us = np.sort([1000.0 * begin.elapsed_time(end) for begin, end in events])
        return [round(float(np.percentile(us, q)), 1) for q in (50, 10, 90)]


def quality(ctx, rows):
    ctx.set_motion_estimator(capi.ESTIMATOR_PYRAMID)
    ctx.set_interpolator(capi.INTERPOLATOR_COMPENSATED, 48)
    w, h = SIZES["1080p"]
    for name, base in (("B", fill_model.SCENE_B), ("A", fill_model.SCENE_A)):
        k = h / base["h"]
        sc = dict(base, w=w, h=h, sq=int(base["sq"] * k), at=(int(base["at"][0] * k), int(base["at"][1] * k)))
        (prev, truth, curr), _ = fill_model.fast_scene(**sc)
        p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
        r = {"row": "quality", "scene": f"{name} at 1920x1080, square {sc['sq']} at {sc['at']}, pan {sc['pan']}, shift {sc['shift']}"}
        for reach in (-1, 16, 32, 64, 255):
            ctx.set_hole_reach(reach)
            ctx.interpolate_frames(p, c, o, 0.5)
            r["off" if reach < 0 else f"reach{reach}"] = fill_model.wrong_pixels(ctx.download(o), truth)
        ctx.set_hole_reach(-1)
        emit(rows, r)
        for f in (p, c, o):
            ctx.destroy_frame(f)
    ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
    ctx.set_interpolator(capi.INTERPOLATOR_SHADER, 48)


def main():
    a = arguments("1080p,4k")
    rows = []
    stream = torch.cuda.Stream()
    with capi.Context(0, stream=stream.cuda_stream) as ctx:
        time = Timer(ctx, stream, a.calls, a.warmup)
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for name, prev, curr, vectors in contents(w, h):
                p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
                if vectors is None:
                    m = ctx.create_frame(w, h, MV)
                    ctx.motion(p, c, m)
                else:
                    m = ctx.frame_from(vectors, MV)
                r = {"row": "calls", "size": size, "content": name}
                for reach in REACHES:
                    ctx.set_hole_reach(reach)
                    r["off_us" if reach < 0 else f"reach{reach}_us"] = time(lambda: ctx.interpolate_compensated(p, c, m, o, 0.5, 48))
                ctx.set_hole_reach(-1)
                emit(rows, r)
                for f in (p, c, m, o):
                    ctx.destroy_frame(f)
            k, pl = ctx.frame_from(border_donors(w, h)), ctx.create_frame(w, h)
            r = {"row": "growth", "size": size, "content": "all holes, donors on the border"}
            for reach in (16, 255):
                r[f"reach{reach}_us"] = time(lambda: ctx.hole_fill_plane(k, pl, reach))
            r["ratio"] = round(r["reach255_us"][0] / r["reach16_us"][0], 2)
            emit(rows, r)
            ctx.destroy_frame(k)
            ctx.destroy_frame(pl)
        quality(ctx, rows)
    for size in a.sizes.split(","):
        w, h = SIZES[size]
        for band in BANDS:
            os.environ["LFG_FILL_BAND"] = str(band)
            with capi.Context(0, stream=stream.cuda_stream) as ctx:
                time = Timer(ctx, stream, a.calls, a.warmup)
                k, pl = ctx.frame_from(border_donors(w, h)), ctx.create_frame(w, h)
                r = {"row": "band", "size": size, "band": band}
                for reach in (16, 255):
                    r[f"reach{reach}_us"] = time(lambda: ctx.hole_fill_plane(k, pl, reach))
                emit(rows, r)
            del os.environ["LFG_FILL_BAND"]
    write_json(a.json, rows)


if __name__ == "__main__":
    main()
