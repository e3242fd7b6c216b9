"""lfg_deband on the GPU, byte for byte against the CPU model (tests/deband_model.py): the smallest shapes that can go wrong under
every layout that changes the route (the 16-byte kernel, its remainder launch, the dword kernel), sentinels around every row,
views, every parameter at both ends, three lanes, argument checks, and that the call leaves no state behind."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import deband_model as dm
from tests.gpu_kit import ctx, three_lanes
from tests.test_gpu_sharpen import Plane, layouts

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (63, 5), (64, 4), (65, 9), (67, 33), (200, 120), (257, 131)]
ITERATIONS, THRESHOLDS, RADII, GRAINS, SEEDS = (1, 2, 3, 4), (0, 4, 64), (1, 16, 32), (0, 3, 16), (0, 1, 0xFFFFFFFF)


def check(ctx, frame, settings, name, layout):
    """`frame` through lfg_deband under every (I, T, R, G, seed) of `settings` and this layout: the model's bytes, the input as
    it was, the output's padding and surroundings still SENTINEL."""
    (in_pitch, in_lead), (out_pitch, out_lead) = layout
    h, w = frame.shape[:2]
    src, dst = Plane(ctx, h, w * 4, in_pitch, in_lead, frame), Plane(ctx, h, w * 4, out_pitch, out_lead)
    try:
        for k, (I, T, R, G, seed) in enumerate(settings):
            if k:
                dst.reset()
            ctx.deband(src.as_frame(w, h), dst.as_frame(w, h), I, T, R, G, seed)
            got, want = dst.fetch(f"{w}x{h} {name}").reshape(h, w, 4), dm.deband(frame, I, T, R, G, seed)
            assert (got == want).all(), (f"{w}x{h} I={I} T={T} R={R} G={G} seed={seed} layout {name}: {int((got != want).sum())} bytes differ, "
                                         f"first at {np.argwhere(got != want)[:3].tolist()}")
        assert src.unchanged()
    finally:
        src.free()
        dst.free()


def rotating(start, count):
    """`count` settings, every I in turn, the other parameters walking through their lists at different paces."""
    return [(ITERATIONS[k % 4], THRESHOLDS[k % 3], RADII[(k // 3) % 3], GRAINS[(k // 2) % 3], SEEDS[(k // 4) % 3]) for k in range(start, start + count)]


# ---- 1. bytes equal the model: shapes x layouts x parameters

@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_equals_the_model(ctx, w, h):
    """Both routes under twelve settings each (every I three times over, every T, R, G and seed), the mixed layouts under four."""
    frame = dm.scene(w, h, 100 * w + h)
    for n, (name, layout) in enumerate(layouts(w).items()):
        check(ctx, frame, rotating(5 * n, 12 if name in ("aligned", "dword") else 4), name, layout)


def test_every_parameter_combination(ctx):
    """I x T x R x G in full at 65 x 9 -- one wide launch and its remainder column -- the seeds in turn."""
    frame = dm.scene(65, 9, 77)
    settings = [(I, T, R, G, SEEDS[k % 3]) for k, (I, T, R, G) in
                enumerate((I, T, R, G) for I in ITERATIONS for T in THRESHOLDS for R in RADII for G in GRAINS)]
    assert len(settings) == 108
    check(ctx, frame, settings, "aligned", layouts(65)["aligned"])


def test_1080p(ctx):
    frame = np.tile(dm.scene(480, 270, 5), (4, 4, 1))
    assert frame.shape == (1080, 1920, 4)
    f, o = ctx.frame_from(frame), ctx.create_frame(1920, 1080)
    try:
        ctx.deband(f, o, 4, 4, 16, 3, 1)
        got, want = ctx.download(o), dm.deband(frame, 4, 4, 16, 3, 1)
        assert (got == want).all(), f"{int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


def test_seeds_differ_and_repeat(ctx):
    frame = dm.ramp(200, 16)[0]
    f, o = ctx.frame_from(frame), ctx.create_frame(200, 16)
    try:
        outs = []
        for seed in (1, 2, 1):
            ctx.deband(f, o, 2, 4, 16, 3, seed)
            outs.append(ctx.download(o))
        assert (outs[0] == outs[2]).all() and (outs[0] != outs[1]).any()
        assert (outs[0] == dm.deband(frame, 2, 4, 16, 3, 1)).all() and (outs[1] == dm.deband(frame, 2, 4, 16, 3, 2)).all()
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


# ---- 2. a view is its own image: nothing outside it is read or written

@pytest.mark.parametrize("x0,y0", [(8, 2), (1, 1)], ids=["aligned", "unaligned"])
def test_region_of_interest(ctx, x0, y0):
    """R I = 128 reaches far beyond the view on every side: the taps clamp to the view, whatever lies around it."""
    big_w, big_h, w, h = 40, 12, 13, 7
    inside = dm.scene(w, h, 77)
    results = []
    for outside in (0xFF, 0x00):
        big = np.full((big_h, big_w, 4), outside, np.uint8)
        big[y0:y0 + h, x0:x0 + w] = inside
        src = Plane(ctx, big_h, big_w * 4, big_w * 4, 0, big)
        dst = Plane(ctx, h, w * 4, big_w * 4, (y0 * big_w + x0) * 4)          # the same window of another frame of that size
        try:
            view = capi.Context.wrap(src.frame.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
            ctx.deband(view, dst.as_frame(w, h), 4, 64, 32, 3, 9)
            results.append(dst.fetch("roi").reshape(h, w, 4))
            assert src.unchanged()
        finally:
            src.free()
            dst.free()
    assert (results[0] == results[1]).all()
    assert (results[0] == dm.deband(inside, 4, 64, 32, 3, 9)).all()


# ---- 3. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 16, 6
    src = Plane(ctx, h + 2, w * 4, w * 4 + 16, 16, dm.scene(w, h + 2, 5))
    dst = Plane(ctx, h, w * 4, w * 4 + 16, 16)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        good_in, good_out = src.as_frame(w, h), dst.as_frame(w, h)
        ok = (2, 4, 16, 3, 7)

        def framed(like, ptr=None, width=w, height=h, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height, f.pitch, f.format = like.data if ptr is None else ptr, width, height, pitch or like.pitch, capi.FORMAT_RGBA8
            return f

        no_data = framed(good_in)
        no_data.data = None
        frames = [(None, B(good_in), B(good_out)), (ctx.h, None, B(good_out)), (ctx.h, B(good_in), None),
                  (ctx.h, B(no_data), B(good_out)), (ctx.h, B(good_in), B(no_data)),
                  (ctx.h, B(mv), B(good_out)), (ctx.h, B(good_in), B(mv)),                                 # a wrong format on either side
                  (ctx.h, B(framed(good_in, width=w - 1)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, height=h - 1))),
                  (ctx.h, B(framed(good_in, ptr=good_in.data + 2)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, ptr=good_out.data + 2))),
                  (ctx.h, B(framed(good_in, pitch=w * 4 + 2)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, pitch=w * 4 + 2))),
                  (ctx.h, B(good_in), B(good_in)),                                                         # in place
                  (ctx.h, B(good_in), B(framed(good_in, ptr=good_in.data + good_in.pitch)))]               # out one row into in
        calls = [c + ok for c in frames]
        for at, (lo, hi) in enumerate(((1, 4), (0, 64), (1, 32), (0, 16))):                                # one past each end
            for bad in (lo - 1, hi + 1):
                calls.append((ctx.h, B(good_in), B(good_out)) + ok[:at] + (bad,) + ok[at + 1:])
        results = [lib.lfg_deband(*c) for c in calls]
        assert len(results) == 23 and all(rc == capi.ERR_INVALID for rc in results), results
        assert lib.lfg_last_error(ctx.h).decode().startswith("lfg_deband:")
        ctx.sync()
        assert src.unchanged() and dst.unchanged()
        for I, T, R, G in ((1, 0, 1, 0), (4, 64, 32, 16)):                                                 # both ends themselves are valid
            dst.reset()
            ctx.deband(good_in, good_out, I, T, R, G, 7)
            want = dm.deband(src.view(src.host)[:h].reshape(h, w, 4), I, T, R, G, 7)
            assert (dst.fetch("valid").reshape(h, w, 4) == want).all()
    finally:
        ctx.destroy_frame(mv)
        src.free()
        dst.free()


# ---- 4. three lanes

def test_three_lanes_give_the_same(ctx):
    sizes = [(67, 9), (64, 4), (13, 7), (130, 33), (5, 3), (256, 17)]
    inputs = [(dm.scene(w, h, 900 + i),) for i, (w, h) in enumerate(sizes)]
    settings = rotating(1, len(sizes))
    alone = []
    for (frame,), s in zip(inputs, settings):
        h, w = frame.shape[:2]
        f, o = ctx.frame_from(frame), ctx.create_frame(w, h)
        ctx.deband(f, o, *s)
        alone.append(ctx.download(o))
        assert (alone[-1] == dm.deband(frame, *s)).all()
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)

    def enqueue(i, frame):
        h, w = frame.shape[:2]
        f, o = ctx.frame_from(frame), ctx.create_frame(w, h)
        ctx.deband(f, o, *settings[i])
        return f, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- 5. the call leaves no state

def test_interpolation_is_what_it_was_before_the_call(ctx):
    """Every opt-in switch at its default: lfg_interpolate_frames on the lane gives the same bytes before and after lfg_deband."""
    w, h = 96, 64
    prev = synth.make_prev(w, h, synth.BASE_SEED)
    curr = synth.translate(prev, (3, -2), synth.BASE_SEED + 1)
    p, c, o, d = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h), ctx.create_frame(w, h)
    try:
        ctx.interpolate_frames(p, c, o, 0.5)
        before = ctx.download(o)
        ctx.deband(c, d, 4, 64, 32, 16, 3)
        assert (ctx.download(d) == dm.deband(curr, 4, 64, 32, 16, 3)).all()
        ctx.upload(o, np.zeros_like(before))
        ctx.interpolate_frames(p, c, o, 0.5)
        assert (ctx.download(o) == before).all()
        assert (ctx.download(p) == prev).all() and (ctx.download(c) == curr).all()
    finally:
        for f in (p, c, o, d):
            ctx.destroy_frame(f)
