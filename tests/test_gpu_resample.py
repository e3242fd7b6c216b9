"""lfg_resample on the GPU, byte for byte against the CPU model (tests/resample_model.py) run on the library's own tables: the
smallest shapes at which each path can break, under every layout, with sentinels around every row; every output height around
the tile; the downscales that force few rows per tile; regions of interest; argument checks; three lanes -- and lfg_host
--scale-filter, whose presented frames must be the model of its input frames."""
import ctypes
import functools

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import resample_model as rm
from tests import sharpen_model as sm
from tests.gpu_kit import apply, ctx, host_run, three_lanes

pytestmark = pytest.mark.gpu

SENTINEL = rm.SENTINEL


@functools.lru_cache(maxsize=None)
def taps(filt, n_in, n_out):
    """The library's table of one axis, or None where it refuses."""
    try:
        return capi.resample_taps(filt, n_in, n_out)
    except capi.LfgError as e:
        assert e.code == capi.ERR_UNSUPPORTED
        return None


def model(frame, ow, oh, filt):
    h, w = frame.shape[:2]
    return rm.resample_int(frame, taps(filt, w, ow), taps(filt, h, oh))


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


def check(ctx, frame, ow, oh, filters, layout):
    """`frame` through lfg_resample to ow x oh under every filter and this layout: the model's bytes, the input as it was, the
    output's padding still SENTINEL.  A filter whose table the library refuses must return LFG_ERR_UNSUPPORTED and write nothing."""
    h, w = frame.shape[:2]
    (in_pitch, in_lead), (out_pitch, out_lead) = rm.layouts(w)[layout], rm.layouts(ow)[layout]
    src, dst = Plane(ctx, h, w * 4, in_pitch, in_lead, frame), Plane(ctx, oh, ow * 4, out_pitch, out_lead)
    try:
        dirty = False
        for filt in filters:
            what = f"{w}x{h}->{ow}x{oh} {rm.NAMES[filt]} layout {layout}"
            if dirty:
                dst.reset()
            if taps(filt, w, ow) is None or taps(filt, h, oh) is None:
                rc = ctx.lib.lfg_resample(ctx.h, ctypes.byref(src.as_frame(w, h)), ctypes.byref(dst.as_frame(ow, oh)), filt)
                assert rc == capi.ERR_UNSUPPORTED and ctx.lib.lfg_last_error(ctx.h).decode(), what
                ctx.sync()
                assert dst.unchanged(), what
                dirty = False
                continue
            ctx.resample(src.as_frame(w, h), dst.as_frame(ow, oh), filt)
            dirty = True
            got, want = dst.fetch(what).reshape(oh, ow, 4), model(frame, ow, oh, filt)
            assert (got == want).all(), f"{what}: {int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"
        assert src.unchanged()
    finally:
        src.free()
        dst.free()


# ---- 1. bytes equal the model: shapes x layouts x filters x contents

@pytest.mark.parametrize("shape", rm.SHAPES, ids=["{}x{}-{}x{}".format(*s) for s in rm.SHAPES])
def test_equals_the_model(ctx, shape):
    w, h, ow, oh = shape
    for layout in rm.layouts(w):
        check(ctx, sm.smooth_scene(w, h, 100 * w + h), ow, oh, rm.FILTERS, layout)
        check(ctx, sm.noise(w, h, 200 * w + h), ow, oh, rm.FILTERS, layout)


def test_every_output_height_around_the_tile(ctx):
    """13 x 40 -> 17 x h for h = 1 .. 2 T + 1, T = 16 from the plan of each table: a tile one row short, full, one row into the
    next, two tiles and a row.  Below 4 rows (2 under the triangle) the ratio is past 64 taps: refused, nothing written."""
    frame = sm.noise(13, 40, 7)
    for oh in range(1, 2 * 16 + 2):
        for filt in rm.FILTERS:
            t = taps(filt, 40, oh)
            assert (t is None) == (rm.table(filt, 40, oh) is None)
            assert t is None or rm.plan_rows(t[0], t[1])[0] == 16
        check(ctx, frame, 17, oh, rm.FILTERS, "dword")


@pytest.mark.parametrize("rows", [4, 2, 1])
def test_downscales_that_force_few_rows_per_tile(ctx, rows):
    """8 x 110 / 160 / 200 -> 8 x 20: under Lanczos-3 the plan is T = 4 / 2 / 1.  One row fewer leaves a last tile that is not full."""
    w, h, ow, oh = rm.SMALL_T[rows]
    t = taps(rm.LANCZOS3, h, oh)
    assert rm.plan_rows(t[0], t[1])[0] == rows
    frame = sm.noise(w, h, 30 + rows)
    check(ctx, frame, ow, oh, rm.FILTERS, "dword")
    check(ctx, frame, ow, oh - 1, rm.FILTERS, "tight")


def test_a_source_of_64_rows(ctx):
    """8 x 64 -> 8 x h down to 64 taps per row: a source of 64 rows fits a tile's LDS rows whole, the plan stays at T = 16."""
    frame = rm.binary_noise(8, 64, 11)
    for oh in (32, 13, 8, 7, 6):
        t = taps(rm.LANCZOS3, 64, oh)
        assert rm.plan_rows(t[0], t[1])[0] == 16
        check(ctx, frame, 8, oh, rm.FILTERS, "dword")


# ---- 2. a region of interest: nothing outside the view is read or written

@pytest.mark.parametrize("ow,oh", [(17, 10), (5, 3)], ids=["up", "down"])
def test_region_of_interest(ctx, ow, oh):
    big_w, big_h, w, h, x0, y0 = 40, 12, 13, 7, 3, 2
    inside = sm.smooth_scene(w, h, 77)
    for filt in (rm.BILINEAR, rm.LANCZOS3):
        results = []
        for outside in (0xFF, 0x00):
            big = np.full((big_h, big_w, 4), outside, np.uint8)
            big[y0:y0 + h, x0:x0 + w] = inside
            src = Plane(ctx, big_h, big_w * 4, big_w * 4, 0, big)
            dst = Plane(ctx, oh, ow * 4, big_w * 4, (y0 * big_w + x0) * 4)      # a window of another frame of that size
            try:
                view = capi.Context.wrap(src.frame.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
                ctx.resample(view, dst.as_frame(ow, oh), filt)
                results.append(dst.fetch("roi").reshape(oh, ow, 4))
                assert src.unchanged()
            finally:
                src.free()
                dst.free()
        assert (results[0] == results[1]).all()
        assert (results[0] == model(inside, ow, oh, filt)).all()


# ---- 3. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h, ow, oh = 16, 6, 24, 9
    src = Plane(ctx, h + 2, w * 4, w * 4 + 16, 16, sm.noise(w, h + 2, 5))
    dst = Plane(ctx, oh, ow * 4, ow * 4 + 16, 16)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    F = capi.FILTER_CATMULL_ROM
    try:
        good_in, good_out = src.as_frame(w, h), dst.as_frame(ow, oh)

        def framed(like, ptr=None, width=None, height=None, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height = like.data if ptr is None else ptr, like.width if width is None else width, like.height if height is None else height
            f.pitch, f.format = pitch or like.pitch, capi.FORMAT_RGBA8
            return f

        no_data = framed(good_in)
        no_data.data = None
        calls = [(None, B(good_in), B(good_out), F), (ctx.h, None, B(good_out), F), (ctx.h, B(good_in), None, F),
                 (ctx.h, B(no_data), B(good_out), F), (ctx.h, B(good_in), B(no_data), F),
                 (ctx.h, B(mv), B(good_out), F), (ctx.h, B(good_in), B(mv), F),                             # MV_S8X2 on either side
                 (ctx.h, B(framed(good_in, width=0)), B(good_out), F), (ctx.h, B(good_in), B(framed(good_out, height=0)), F),
                 (ctx.h, B(framed(good_in, ptr=good_in.data + 2)), B(good_out), F), (ctx.h, B(good_in), B(framed(good_out, ptr=good_out.data + 2)), F),
                 (ctx.h, B(framed(good_in, pitch=w * 4 + 2)), B(good_out), F), (ctx.h, B(good_in), B(framed(good_out, pitch=ow * 4 + 2)), F),
                 (ctx.h, B(framed(good_in, pitch=w * 4 - 4)), B(good_out), F), (ctx.h, B(good_in), B(framed(good_out, pitch=ow * 4 - 4)), F),
                 (ctx.h, B(good_in), B(good_in), F),                                                        # in place
                 (ctx.h, B(good_in), B(framed(good_in, ptr=good_in.data + good_in.pitch)), F),              # out one row into in
                 (ctx.h, B(good_in), B(good_out), -1), (ctx.h, B(good_in), B(good_out), 6)]                 # unknown filters
        results = [lib.lfg_resample(*c) for c in calls]
        assert all(rc == capi.ERR_INVALID for rc in results), results
        assert lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert src.unchanged() and dst.unchanged()
        ctx.resample(good_in, good_out, F)                        # a valid call next to the bad ones works
        want = model(src.view(src.host)[:h].reshape(h, w, 4), ow, oh, F)
        assert (dst.fetch("valid").reshape(oh, ow, 4) == want).all()
    finally:
        ctx.destroy_frame(mv)
        src.free()
        dst.free()


def test_timed_as_the_scale_stage_and_leaves_the_last_kernel_alone(ctx):
    frame = sm.noise(13, 7, 1)
    f, o = ctx.frame_from(frame), ctx.create_frame(17, 10)
    try:
        before = ctx.lib.lfg_scale_last_kernel(ctx.h)
        launches = ctypes.c_uint64()
        assert ctx.lib.lfg_profile_enable(ctx.h, 1) == 0 and ctx.lib.lfg_profile_reset(ctx.h) == 0
        ctx.resample(f, o, capi.FILTER_MITCHELL)
        assert ctx.lib.lfg_profile_get(ctx.h, capi.STAGE_SCALE, None, ctypes.byref(launches)) == 0 and launches.value == 1
        assert ctx.lib.lfg_scale_last_kernel(ctx.h) == before
    finally:
        ctx.lib.lfg_profile_enable(ctx.h, 0)
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


def test_more_tables_than_the_context_keeps(ctx):
    """20 sizes, 40 tables: the bounded cache drops the oldest, and a size seen before is built again and gives the same bytes."""
    frame = sm.noise(13, 7, 2)
    f = ctx.frame_from(frame)
    try:
        for ow in list(range(14, 34)) + [14]:
            o = ctx.create_frame(ow, ow - 5)
            ctx.resample(f, o, capi.FILTER_LANCZOS2)
            assert (ctx.download(o) == model(frame, ow, ow - 5, rm.LANCZOS2)).all(), ow
            ctx.destroy_frame(o)
    finally:
        ctx.destroy_frame(f)


# ---- 4. three lanes

def test_three_lanes_give_the_same(ctx):
    cases = [(67, 9, 130, 20, rm.LANCZOS3), (64, 9, 8, 3, rm.BILINEAR), (13, 7, 26, 14, rm.CATMULL_ROM), (130, 33, 70, 11, rm.MITCHELL),
             (5, 3, 11, 8, rm.NEAREST), (96, 17, 200, 40, rm.LANCZOS2)]
    inputs = [(sm.smooth_scene(w, h, 900 + i),) for i, (w, h, _, _, _) in enumerate(cases)]
    alone = []
    for (frame,), (w, h, ow, oh, filt) in zip(inputs, cases):
        f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
        ctx.resample(f, o, filt)
        alone.append(ctx.download(o))
        assert (alone[-1] == model(frame, ow, oh, filt)).all()
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)

    def enqueue(i, frame):
        _, _, ow, oh, filt = cases[i]
        f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
        ctx.resample(f, o, filt)
        return f, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- 5. lfg_host --scale-filter

COMPENSATED = ("--semantics", "intended", "--interpolator", "compensated")


@pytest.fixture(scope="module")
def frames():
    """Three synth frames of 24 x 16."""
    out = [synth.make_prev(24, 16, synth.BASE_SEED)]
    for k in (1, 2):
        out.append(synth.translate(out[-1], (2, -1), synth.BASE_SEED + k))
    return out


@pytest.mark.parametrize("size", [(48, 32), (12, 8)], ids=["up", "down"])
def test_host_presents_the_model_under_every_filter(frames, tmp_path, size):
    for filt in rm.FILTERS:
        info, got = host_run(tmp_path / rm.NAMES[filt], frames, size, "--no-interpolation", "--scale-filter", rm.NAMES[filt])
        assert info["scale_filter"] == rm.NAMES[filt] and info["presented"] == 3
        for k in range(3):
            assert (got[k] == model(frames[k], *size, filt)).all(), (rm.NAMES[filt], k)


def test_host_generates_from_the_filtered_frames(ctx, frames, tmp_path):
    """Real frames are the model; generated ones are lfg_interpolate_frames of the model's upscaled pair under the same
    settings.  Three frames in flight give the same bytes."""
    options = (*COMPENSATED, "--scale-filter", "catmull-rom")
    info, got = host_run(tmp_path / "two", frames, (48, 32), *options)
    assert info["scale_filter"] == "catmull-rom" and info["presented"] == 5 and info["interpolated"] == 2
    up = [model(f, 48, 32, rm.CATMULL_ROM) for f in frames]
    for k in range(3):
        assert (got[2 * k] == up[k]).all(), k
    apply(ctx, ("full", -1, "compensated", capi.SEMANTICS_INTENDED))
    try:
        for k in range(2):
            p, c, o = ctx.frame_from(up[k]), ctx.frame_from(up[k + 1]), ctx.create_frame(48, 32)
            ctx.interpolate_frames(p, c, o, 0.5)
            want = ctx.download(o)
            for f in (p, c, o):
                ctx.destroy_frame(f)
            assert (got[2 * k + 1] == want).all(), k
    finally:
        apply(ctx, ("full", -1, "shader", capi.SEMANTICS_REFERENCE))
    _, three = host_run(tmp_path / "three", frames, (48, 32), *options, "--in-flight", "3")
    assert (three == got).all()


def test_host_reference_is_the_default(frames, tmp_path):
    info, plain = host_run(tmp_path / "p", frames, (48, 32), *COMPENSATED)
    named, got = host_run(tmp_path / "r", frames, (48, 32), *COMPENSATED, "--scale-filter", "reference")
    assert "scale_filter" not in info and "scale_filter" not in named and (got == plain).all()
    other, filtered = host_run(tmp_path / "l", frames, (48, 32), *COMPENSATED, "--scale-filter", "lanczos3")
    assert other["scale_filter"] == "lanczos3" and (filtered != plain).any()


def test_host_evaluates_under_a_filter(frames, tmp_path):
    """--evaluate --scale-filter lanczos2 runs and reports (host_run reads a raw output: the report alone is what this run has)."""
    import json
    import subprocess

    from tests.gpu_kit import HOST
    src = tmp_path / "in.rgba"
    np.concatenate([f.reshape(-1) for f in frames]).tofile(src)
    p = subprocess.run([HOST, "--input-width", "24", "--input-height", "16", "--output-width", "48", "--output-height", "32", "--frames", "3",
                        "--quiet", "--input-raw", str(src), "--evaluate", "--scale-filter", "lanczos2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["scale_filter"] == "lanczos2" and info["evaluation"]["pairs"] == 1
    assert info["evaluation"]["generated"]["pixels"] > 0
