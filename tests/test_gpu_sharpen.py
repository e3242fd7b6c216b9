"""lfg_sharpen on the GPU, byte for byte against the CPU model (tests/sharpen_model.py): the smallest shapes that can go wrong
under every layout that changes the path (the 16-byte kernel, its remainder launch, the dword kernel), sentinels around every
row, regions of interest, argument checks, three lanes -- and lfg_host --sharpen, whose presented frames must be the model of the
frames it presents without the option."""
import ctypes
import os
import re

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import sharpen_model as sm
from tests import yuv_model as ym
from tests.gpu_kit import ROOT, ctx, host_run, three_lanes

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
SHAPES = [(1, 1), (2, 1), (1, 3), (3, 2), (4, 1), (5, 3), (13, 7), (64, 4), (65, 4), (66, 4), (67, 9)]
STRENGTHS = (0, 1, 16, 37, 64)
# the strip length R of the kernels: every height from 1 to 2 R + 1 takes another way through the strips
STRIP_ROWS = int(re.search(r"constexpr int kSharpenRows = (\d+);", open(os.path.join(ROOT, "linux-fg_amd", "csrc", "sharpen.hip")).read())[1])


def up16(n):
    return (n + 15) // 16 * 16


def layouts(w):
    """name -> ((in pitch, in lead), (out pitch, out lead)).  tight: as lfg_frame_create lays a frame out; dword: nothing is
    16-byte aligned; aligned: bases and pitches multiples of 16 (the 16-byte kernel, with the dword kernel behind it for a width
    that is no multiple of 4); one side aligned and the other not: the dword kernel."""
    tight, odd, aligned = (w * 4, 0), (w * 4 + 4, 4), (up16(w * 4) + 16, 32)
    return {"tight": (tight, tight), "dword": (odd, odd), "aligned": (aligned, (up16(w * 4) + 32, 16)),
            "in-aligned": (aligned, odd), "out-aligned": (odd, aligned)}


class Plane:
    """`rows` rows of `row_bytes` bytes, `pitch` apart, `lead` bytes into device memory that is otherwise SENTINEL (or `fill`).
    fetch() returns the rows and asserts that no other byte has changed."""

    def __init__(self, ctx, rows, row_bytes, pitch, lead, data=None, fill=SENTINEL):
        self.ctx, self.rows, self.row_bytes, self.pitch, self.lead, self.fill = ctx, rows, row_bytes, pitch, lead, fill
        texel_rows = -(-(lead + (rows - 1) * pitch + row_bytes + 64) // 4096)
        self.host = np.full(texel_rows * 4096, fill, np.uint8)
        if data is not None:
            self.view(self.host)[...] = np.ascontiguousarray(data).reshape(rows, row_bytes)
        self.frame = ctx.frame_from(self.host.reshape(texel_rows, 1024, 4))

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.lead:], (self.rows, self.row_bytes), (self.pitch, 1))

    def as_frame(self, w, h):
        return capi.Context.wrap(self.frame.data + self.lead, w, h, pitch=self.pitch)

    def reset(self):
        self.ctx.upload(self.frame, self.host.reshape(-1, 1024, 4))

    def fetch(self, what=""):
        got = self.ctx.download(self.frame).reshape(-1)
        rows = self.view(got).copy()
        self.view(got)[...] = self.fill
        assert (got == self.fill).all(), f"{what}: {int((got != self.fill).sum())} bytes outside the rows were written"
        return rows

    def unchanged(self):
        return (self.ctx.download(self.frame).reshape(-1) == self.host).all()

    def free(self):
        self.ctx.destroy_frame(self.frame)


def check(ctx, frame, strengths, name, layout):
    """`frame` through lfg_sharpen at every strength under this layout: the model's bytes, the input as it was, the output's
    padding still SENTINEL."""
    (in_pitch, in_lead), (out_pitch, out_lead) = layout
    h, w = frame.shape[:2]
    src, dst = Plane(ctx, h, w * 4, in_pitch, in_lead, frame), Plane(ctx, h, w * 4, out_pitch, out_lead)
    try:
        for k, strength in enumerate(strengths):
            if k:
                dst.reset()
            ctx.sharpen(src.as_frame(w, h), dst.as_frame(w, h), strength)
            got, want = dst.fetch(f"{w}x{h} {name}").reshape(h, w, 4), sm.sharpen(frame, strength)
            assert (got == want).all(), (f"{w}x{h} strength {strength} layout {name}: {int((got != want).sum())} bytes differ, "
                                         f"first at {np.argwhere(got != want)[:3].tolist()}")
        assert src.unchanged()
    finally:
        src.free()
        dst.free()


# ---- 1. bytes equal the model: shapes x layouts x strengths x contents

@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_equals_the_model(ctx, w, h):
    for name, layout in layouts(w).items():
        check(ctx, sm.smooth_scene(w, h, 100 * w + h), STRENGTHS, name, layout)
        check(ctx, sm.noise(w, h, 200 * w + h), STRENGTHS, name, layout)


@pytest.mark.parametrize("w", [5, 67])
def test_every_height_around_the_strip_length(ctx, w):
    """1 .. 2 R + 1 rows: a strip one row short, full, one row into the next, two strips and a row."""
    for h in range(1, 2 * STRIP_ROWS + 2):
        for name, layout in layouts(w).items():
            check(ctx, sm.smooth_scene(w, h, 300 * w + h), (37,), name, layout)
            check(ctx, sm.noise(w, h, 400 * w + h), (64,), name, layout)


def test_impulses(ctx):
    """|strength * L| = 65,280: what a 16-bit product would get wrong."""
    for frame in sm.impulses():
        for name, layout in layouts(3).items():
            check(ctx, frame, (64,), name, layout)


# ---- 2. a region of interest: nothing outside the view is read or written

@pytest.mark.parametrize("x0,y0", [(8, 2), (1, 1)], ids=["aligned", "unaligned"])
def test_region_of_interest(ctx, x0, y0):
    big_w, big_h, w, h = 40, 12, 13, 7
    inside = sm.smooth_scene(w, h, 77)
    results = []
    for outside in (0xFF, 0x00):
        big = np.full((big_h, big_w, 4), outside, np.uint8)
        big[y0:y0 + h, x0:x0 + w] = inside
        src = Plane(ctx, big_h, big_w * 4, big_w * 4, 0, big)
        dst = Plane(ctx, h, w * 4, big_w * 4, (y0 * big_w + x0) * 4)          # the same window of another frame of that size
        try:
            view = capi.Context.wrap(src.frame.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
            ctx.sharpen(view, dst.as_frame(w, h), 37)
            results.append(dst.fetch("roi").reshape(h, w, 4))
            assert src.unchanged()
        finally:
            src.free()
            dst.free()
    assert (results[0] == results[1]).all()
    assert (results[0] == sm.sharpen(inside, 37)).all()


# ---- 3. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 16, 6
    src = Plane(ctx, h + 2, w * 4, w * 4 + 16, 16, sm.noise(w, h + 2, 5))
    dst = Plane(ctx, h, w * 4, w * 4 + 16, 16)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        good_in, good_out = src.as_frame(w, h), dst.as_frame(w, h)

        def framed(like, ptr=None, width=w, height=h, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height, f.pitch, f.format = like.data if ptr is None else ptr, width, height, pitch or like.pitch, capi.FORMAT_RGBA8
            return f

        no_data = framed(good_in)
        no_data.data = None
        calls = [(None, B(good_in), B(good_out), 16), (ctx.h, None, B(good_out), 16), (ctx.h, B(good_in), None, 16),
                 (ctx.h, B(no_data), B(good_out), 16), (ctx.h, B(good_in), B(no_data), 16),
                 (ctx.h, B(mv), B(good_out), 16), (ctx.h, B(good_in), B(mv), 16),                         # MV_S8X2 on either side
                 (ctx.h, B(framed(good_in, width=w - 1)), B(good_out), 16), (ctx.h, B(good_in), B(framed(good_out, height=h - 1)), 16),
                 (ctx.h, B(framed(good_in, ptr=good_in.data + 2)), B(good_out), 16), (ctx.h, B(good_in), B(framed(good_out, ptr=good_out.data + 2)), 16),
                 (ctx.h, B(framed(good_in, pitch=w * 4 + 2)), B(good_out), 16), (ctx.h, B(good_in), B(framed(good_out, pitch=w * 4 + 2)), 16),
                 (ctx.h, B(good_in), B(good_in), 16),                                                     # in place
                 (ctx.h, B(good_in), B(framed(good_in, ptr=good_in.data + good_in.pitch)), 16),           # out one row into in
                 (ctx.h, B(good_in), B(good_out), -1), (ctx.h, B(good_in), B(good_out), 65)]
        results = [lib.lfg_sharpen(*c) for c in calls]
        assert all(rc == -1 for rc in results), results           # LFG_ERR_INVALID
        assert lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert src.unchanged() and dst.unchanged()
        ctx.sharpen(good_in, good_out, 16)                        # a valid call next to the bad ones works
        want = sm.sharpen(src.view(src.host)[:h].reshape(h, w, 4), 16)
        assert (dst.fetch("valid").reshape(h, w, 4) == want).all()
    finally:
        ctx.destroy_frame(mv)
        src.free()
        dst.free()


# ---- 4. three lanes

def test_three_lanes_give_the_same(ctx):
    sizes = [(67, 9), (64, 4), (13, 7), (130, 33), (5, 3), (256, 17)]
    inputs = [(sm.smooth_scene(w, h, 900 + i),) for i, (w, h) in enumerate(sizes)]
    strengths = [16, 64, 37, 24, 1, 48]
    alone = []
    for (frame,), strength in zip(inputs, strengths):
        h, w = frame.shape[:2]
        f, o = ctx.frame_from(frame), ctx.create_frame(w, h)
        ctx.sharpen(f, o, strength)
        alone.append(ctx.download(o))
        assert (alone[-1] == sm.sharpen(frame, strength)).all()
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)

    def enqueue(i, frame):
        h, w = frame.shape[:2]
        f, o = ctx.frame_from(frame), ctx.create_frame(w, h)
        ctx.sharpen(f, o, strengths[i])
        return f, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- 5. lfg_host --sharpen

COMPENSATED = ("--semantics", "intended", "--interpolator", "compensated")


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """Three synth frames of 24 x 16 and what lfg_host presents of them at 48 x 32 without the option."""
    w, h = 24, 16
    frames = [synth.make_prev(w, h, synth.BASE_SEED)]
    for k in (1, 2):
        frames.append(synth.translate(frames[-1], (2, -1), synth.BASE_SEED + k))
    info, plain = host_run(tmp_path_factory.mktemp("plain"), frames, (48, 32), *COMPENSATED)
    assert info["presented"] == 5 and "sharpen" not in info
    return frames, plain


def test_host_sharpens_real_and_generated_frames_alike(stream, tmp_path):
    """All five presented frames are the model of the frames presented without the option: the generated ones could not be if
    the motion stage had seen a sharpened frame."""
    frames, plain = stream
    info, got = host_run(tmp_path / "s", frames, (48, 32), *COMPENSATED, "--sharpen", "24")
    assert info["sharpen"] == 24 and info["presented"] == 5 and info["interpolated"] == 2
    for k in range(5):
        want = sm.sharpen(plain[k], 24)
        assert (got[k] == want).all(), k
        assert (want != plain[k]).any(), k                        # (the option does something to every frame)


def test_host_sharpens_with_three_frames_in_flight(stream, tmp_path):
    frames, plain = stream
    _, got = host_run(tmp_path / "s", frames, (48, 32), *COMPENSATED, "--sharpen", "24", "--in-flight", "3")
    assert all((got[k] == sm.sharpen(plain[k], 24)).all() for k in range(5))


def test_host_sharpens_every_factor(stream, tmp_path):
    frames, _ = stream
    factors = ("--factors", "0.25,0.5,0.75")
    info, plain = host_run(tmp_path / "p", frames, (48, 32), *COMPENSATED, *factors)
    sharp_info, got = host_run(tmp_path / "s", frames, (48, 32), *COMPENSATED, *factors, "--sharpen", "24")
    assert info["presented"] == sharp_info["presented"] == 9
    assert all((got[k] == sm.sharpen(plain[k], 24)).all() for k in range(9))


def test_host_sharpen_0_is_the_default(stream, tmp_path):
    frames, plain = stream
    info, got = host_run(tmp_path / "s", frames, (48, 32), *COMPENSATED, "--sharpen", "0")
    assert "sharpen" not in info and (got == plain).all()


def test_host_converts_the_sharpened_frames_to_nv12(stream, tmp_path):
    frames, plain = stream
    mode = (ym.BT709, ym.LIMITED, ym.LEFT)                        # lfg_host's defaults
    _, got = host_run(tmp_path / "s", frames, (48, 32), *COMPENSATED, "--sharpen", "24", "--output-format", "nv12")
    for k in range(5):
        want_y, want_uv = ym.rgba_to_nv12(sm.sharpen(plain[k], 24), *mode)
        assert (got[k][0] == want_y).all() and (got[k][1] == want_uv).all(), k


def test_host_sharpens_at_the_input_size(tmp_path):
    """Presented at the input size (the upscale is then the identity)."""
    frames = [synth.make_prev(24, 16, synth.BASE_SEED)]
    for k in (1, 2):
        frames.append(synth.translate(frames[-1], (2, -1), synth.BASE_SEED + k))
    _, plain = host_run(tmp_path / "p", frames, (24, 16), *COMPENSATED)
    info, got = host_run(tmp_path / "s", frames, (24, 16), *COMPENSATED, "--sharpen", "24")
    assert info["sharpen"] == 24 and len(plain) == len(got) == 5
    assert all((got[k] == sm.sharpen(plain[k], 24)).all() for k in range(5))
