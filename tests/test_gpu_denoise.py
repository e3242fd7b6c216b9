"""lfg_denoise_temporal on the GPU, byte for byte against the CPU model (tests/denoise_model.py): the smallest shapes that can go
wrong at every radius and with one and two references, fields that point anywhere, padded pitches with sentinels around every
output row, regions of interest, the ends of the parameter ranges, every refusal, three lanes -- and a noisy pan filtered
recursively on the vectors of lfg_motion, step by step equal to the model and closer to the clean stream than what went in."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import denoise_cases as dc
from tests import denoise_model as dm
from tests.gpu_kit import ctx, first_bad, three_lanes

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


class Plane:
    """`rows` rows of `row_bytes` bytes, `pitch` apart, `lead` bytes into device memory that is otherwise SENTINEL.  fetch()
    returns the rows and asserts that no other byte has changed."""

    def __init__(self, ctx, rows, row_bytes, pitch, lead, data=None):
        self.ctx, self.rows, self.row_bytes, self.pitch, self.lead = ctx, rows, row_bytes, pitch, lead
        texel_rows = -(-(lead + (rows - 1) * pitch + row_bytes + 64) // 4096)
        self.host = np.full(texel_rows * 4096, SENTINEL, np.uint8)
        if data is not None:
            self.view(self.host)[...] = np.ascontiguousarray(data).view(np.uint8).reshape(rows, row_bytes)
        self.frame = ctx.frame_from(self.host.reshape(texel_rows, 1024, 4))

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.lead:], (self.rows, self.row_bytes), (self.pitch, 1))

    def as_frame(self, w, h, fmt=capi.FORMAT_RGBA8):
        return capi.Context.wrap(self.frame.data + self.lead, w, h, fmt, pitch=self.pitch)

    def reset(self):
        self.ctx.upload(self.frame, self.host.reshape(-1, 1024, 4))

    def fetch(self, what=""):
        got = self.ctx.download(self.frame).reshape(-1)
        rows = self.view(got).copy()
        self.view(got)[...] = SENTINEL
        assert (got == SENTINEL).all(), f"{what}: {int((got != SENTINEL).sum())} bytes outside the rows were written"
        return rows

    def unchanged(self):
        return (self.ctx.download(self.frame).reshape(-1) == self.host).all()

    def free(self):
        self.ctx.destroy_frame(self.frame)


def layouts(w):
    """name -> (RGBA8 (pitch, lead), mv (pitch, lead)): as lfg_frame_create lays frames out, and padded with nothing aligned
    beyond what the call asks for (4 bytes for RGBA8, 2 for vectors)."""
    return {"tight": ((w * 4, 0), (w * 2, 0)), "padded": ((w * 4 + 12, 4), (w * 2 + 6, 2))}


def run_cases(ctx, curr, refs, mvs, cases, layout, what):
    """lfg_denoise_temporal under this layout for every (count, radius, tolerance, strength, limit) of `cases`: the model's
    bytes, the inputs as they were, the output's padding still SENTINEL."""
    (pitch, lead), (mv_pitch, mv_lead) = layout
    h, w = curr.shape[:2]
    planes = [Plane(ctx, h, w * 4, pitch, lead, f) for f in [curr] + refs] + [Plane(ctx, h, w * 2, mv_pitch, mv_lead, m) for m in mvs]
    dst = Plane(ctx, h, w * 4, pitch + 8, lead + 4)
    try:
        c, r, m = planes[0].as_frame(w, h), [p.as_frame(w, h) for p in planes[1:3]], [p.as_frame(w, h, capi.FORMAT_MV_S8X2) for p in planes[3:]]
        for k, (count, radius, tolerance, strength, limit) in enumerate(cases):
            if k:
                dst.reset()
            ctx.denoise_temporal(c, r[:count], m[:count], dst.as_frame(w, h), radius, tolerance, strength, limit)
            got = dst.fetch(f"{w}x{h} {what}").reshape(h, w, 4)
            want = dm.denoise(curr, refs[:count], mvs[:count], radius, tolerance, strength, limit)
            assert (got == want).all(), f"{w}x{h} {what} count {count} radius {radius} ({tolerance}, {strength}, {limit}): {first_bad(got, want)}"
        assert all(p.unchanged() for p in planes)
    finally:
        for p in planes + [dst]:
            p.free()


def frames_for(w, h, seed):
    """curr, a reference close to it (so that weights are neither all 0 nor all alike) and one that is close in half the frame."""
    curr = dc.noisy(dc.scene(w, h, seed), 6, seed + 1)
    near = dc.noisy(dc.scene(w, h, seed), 6, seed + 2)
    mixed = dc.noisy(curr, 12, seed + 3)
    mixed[:, : w // 2] = dc.random_frame(w, h, seed + 4)[:, : w // 2]
    return curr, [near, mixed]


EVERY = [(count, radius, 32, 192, 255) for count in dc.COUNTS for radius in dc.RADII]


# ---- 1. bytes equal the model: shapes x radii x counts x fields x layouts

@pytest.mark.parametrize("w,h", dc.SHAPES, ids=[f"{w}x{h}" for w, h in dc.SHAPES])
def test_equals_the_model(ctx, w, h):
    curr, refs = frames_for(w, h, 10 * w + h)
    fields = dc.fields(w, h, 20 * w + h)
    for name, field in fields.items():
        other = fields["random"] if name != "random" else dc.small_field(w, h, 30 * w + h)
        for layout_name, layout in layouts(w).items():
            run_cases(ctx, curr, refs, [field, other], EVERY, layout, f"{name} {layout_name}")


def test_a_smooth_field_mixes(ctx):
    """What the cases above leave thin: vectors of a few pixels on content that fits, so that most weights are large."""
    w, h = 65, 5
    curr, refs = frames_for(w, h, 77)
    run_cases(ctx, curr, [refs[0], dc.noisy(curr, 3, 78)], [dc.small_field(w, h, 79, 1), dc.constant_field(w, h, 0, 0)], EVERY, layouts(w)["padded"], "smooth")


# ---- 2. the ends of the parameter ranges

@pytest.mark.parametrize("w,h", [(3, 2), (65, 5)])
def test_parameter_extremes(ctx, w, h):
    curr, refs = frames_for(w, h, 40 * w + h)
    mvs = [dc.small_field(w, h, 41, 1), dc.constant_field(w, h, 0, 0)]
    cases = [(count, radius, t, s, l) for count in dc.COUNTS for radius in dc.RADII for t, s, l in dc.EXTREMES]
    run_cases(ctx, curr, refs, mvs, cases + [(2, 1, 32, 0, 255), (2, 1, 32, 256, 0)], layouts(w)["padded"], "extremes")
    same = [(count, radius, t, 256, 255) for count in dc.COUNTS for radius in dc.RADII for t in (1, 1020)]
    run_cases(ctx, curr, [curr, curr], mvs[1:] * 2, same, layouts(w)["tight"], "identical")      # cost 0: the largest weights


# ---- 3. a region of interest: nothing outside the views is read or written

@pytest.mark.parametrize("x0,y0", [(8, 2), (1, 1)], ids=["aligned", "unaligned"])
def test_region_of_interest(ctx, x0, y0):
    big_w, big_h, w, h = 40, 12, 13, 7
    curr, refs = frames_for(w, h, 55)
    mvs = [dc.random_field(w, h, 56), dc.outward_field(w, h)]
    want = dm.denoise(curr, refs, mvs, 2, 32, 192, 255)
    for outside in (0xFF, 0x00):
        bigs = []
        for inside in [curr] + refs:
            big = np.full((big_h, big_w, 4), outside, np.uint8)
            big[y0:y0 + h, x0:x0 + w] = inside
            bigs.append(Plane(ctx, big_h, big_w * 4, big_w * 4, 0, big))
        for inside in mvs:
            big = np.full((big_h, big_w, 2), outside, np.uint8)
            big[y0:y0 + h, x0:x0 + w] = inside.view(np.uint8)
            bigs.append(Plane(ctx, big_h, big_w * 2, big_w * 2, 0, big))
        dst = Plane(ctx, h, w * 4, big_w * 4, (y0 * big_w + x0) * 4)          # the same window of another frame of that size
        try:
            views = [capi.Context.wrap(p.frame.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4) for p in bigs[:3]]
            fields = [capi.Context.wrap(p.frame.data + (y0 * big_w + x0) * 2, w, h, capi.FORMAT_MV_S8X2, pitch=big_w * 2) for p in bigs[3:]]
            ctx.denoise_temporal(views[0], views[1:], fields, dst.as_frame(w, h), 2, 32, 192, 255)
            got = dst.fetch("roi").reshape(h, w, 4)
            assert (got == want).all(), first_bad(got, want)
            assert all(p.unchanged() for p in bigs)
        finally:
            for p in bigs + [dst]:
                p.free()


# ---- 4. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 16, 6
    curr, refs = frames_for(w, h + 2, 5)
    mvs = [dc.small_field(w, h + 2, 6), dc.constant_field(w, h + 2, 0, 0)]
    planes = [Plane(ctx, h + 2, w * 4, w * 4 + 16, 16, f) for f in [curr] + refs] + [Plane(ctx, h + 2, w * 2, w * 2 + 8, 8, m) for m in mvs]
    dst = Plane(ctx, h, w * 4, w * 4 + 16, 16)
    q2 = ctx.create_frame(w, h, capi.FORMAT_MV_S16X2_Q2)
    try:
        c, r0, r1 = (p.as_frame(w, h) for p in planes[:3])
        m0, m1 = (p.as_frame(w, h, capi.FORMAT_MV_S8X2) for p in planes[3:])
        out = dst.as_frame(w, h)

        def framed(like, ptr=None, width=w, height=h, pitch=None, fmt=None):
            f = capi.Frame()
            f.data, f.width, f.height, f.pitch = like.data if ptr is None else ptr, width, height, pitch or like.pitch
            f.format = like.format if fmt is None else fmt
            return f

        def no_data(like):
            f = framed(like)
            f.data = None
            return f

        def call(curr=c, refs=(r0, r1), mvs=(m0, m1), count=2, out=out, radius=1, tolerance=32, strength=192, limit=255, handle=ctx.h):
            arr = lambda fs: None if fs is None else (capi._FP * len(fs))(*[None if f is None else ctypes.pointer(f) for f in fs])
            return lib.lfg_denoise_temporal(handle, None if curr is None else B(curr), arr(refs), arr(mvs), count, None if out is None else B(out),
                                            radius, tolerance, strength, limit)

        results = [
            call(handle=None), call(curr=None), call(out=None), call(refs=None), call(mvs=None),
            call(refs=(r0, None)), call(mvs=(m0, None)), call(refs=(None,), mvs=(m0,), count=1),
            call(curr=no_data(c)), call(out=no_data(out)), call(refs=(no_data(r0), r1)), call(mvs=(m0, no_data(m1))),
            call(count=0), call(count=3), call(count=-1),
            call(curr=m0), call(out=m0), call(refs=(m0, r1)), call(mvs=(r0, m1)), call(mvs=(m0, r1)),      # a format in the wrong place
            call(mvs=(q2, m1)), call(mvs=(m0, q2)), call(mvs=(q2,), refs=(r0,), count=1),                 # quarter-pixel fields
            call(curr=framed(c, width=w - 1)), call(out=framed(out, height=h - 1)), call(refs=(r0, framed(r1, width=w - 1))),
            call(mvs=(framed(m0, height=h - 1), m1)),
            call(curr=framed(c, ptr=c.data + 2)), call(out=framed(out, ptr=out.data + 2)), call(refs=(framed(r0, ptr=r0.data + 2), r1)),
            call(mvs=(m0, framed(m1, ptr=m1.data + 1))),
            call(curr=framed(c, pitch=w * 4 + 2)), call(out=framed(out, pitch=w * 4 + 2)), call(refs=(r0, framed(r1, pitch=w * 4 + 2))),
            call(mvs=(framed(m0, pitch=w * 2 + 1), m1)),
            call(out=c), call(out=r0), call(out=r1),                                                      # in place
            call(out=framed(c, ptr=c.data + c.pitch)), call(out=framed(r1, ptr=r1.data + r1.pitch)),      # one row into an input
            call(out=framed(out, ptr=m0.data, pitch=w * 4)), call(out=framed(out, ptr=m1.data, pitch=w * 4)),   # over a field
            call(radius=-1), call(radius=3), call(tolerance=0), call(tolerance=1021), call(strength=-1), call(strength=257),
            call(limit=-1), call(limit=256),
        ]
        assert all(rc == -1 for rc in results), results           # LFG_ERR_INVALID
        assert lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert all(p.unchanged() for p in planes) and dst.unchanged()
        assert call() == 0                                         # a valid call next to the bad ones works
        want = dm.denoise(curr[:h], [f[:h] for f in refs], [m[:h] for m in mvs], 1, 32, 192, 255)
        assert (dst.fetch("valid").reshape(h, w, 4) == want).all()
    finally:
        ctx.destroy_frame(q2)
        for p in planes + [dst]:
            p.free()


# ---- 5. three lanes

def test_three_lanes_give_the_same(ctx):
    sizes = [(67, 9), (64, 4), (13, 7), (130, 33), (5, 3), (256, 17)]
    params = [(1, 1, 32, 192, 255), (2, 2, 32, 64, 255), (2, 0, 100, 256, 3), (2, 1, 16, 192, 255), (1, 2, 1020, 1, 255), (2, 2, 32, 192, 8)]
    inputs = []
    for i, (w, h) in enumerate(sizes):
        curr, refs = frames_for(w, h, 900 + i)
        inputs.append((curr, refs[0], refs[1], dc.small_field(w, h, 950 + i), dc.random_field(w, h, 960 + i)))

    def enqueue(i, curr, r0, r1, m0, m1):
        count, radius, tolerance, strength, limit = params[i]
        h, w = curr.shape[:2]
        fs = [ctx.frame_from(f) for f in (curr, r0, r1)] + [ctx.frame_from(m, capi.FORMAT_MV_S8X2) for m in (m0, m1)] + [ctx.create_frame(w, h)]
        ctx.denoise_temporal(fs[0], fs[1:3][:count], fs[3:5][:count], fs[5], radius, tolerance, strength, limit)
        return fs

    alone = []
    for i, arrays in enumerate(inputs):
        fs = enqueue(i, *arrays)
        alone.append(ctx.download(fs[-1]))
        count, radius, tolerance, strength, limit = params[i]
        curr, r0, r1, m0, m1 = arrays
        assert (alone[-1] == dm.denoise(curr, [r0, r1][:count], [m0, m1][:count], radius, tolerance, strength, limit)).all(), i
        for f in fs:
            ctx.destroy_frame(f)
    three_lanes(ctx, inputs, enqueue, alone)


# ---- 6. end to end: a noisy pan, filtered recursively on the vectors of lfg_motion

def sse(ctx, a, b, record):
    ctx.frame_diff(a, b, record, 0x7)
    return sum(ctx.read_diff_record(record)[1][:3])


def test_a_noisy_pan_filtered_recursively(ctx):
    """128 x 72, a pan by (3, -2) with +-4 levels of noise, six frames: each step's vectors come from lfg_motion(previous output,
    noisy frame) on the device and go, downloaded, to the model; device and model are equal at every step, and the last output
    is closer to the clean frame than the noisy frame it was made of, by lfg_frame_diff's squared sums."""
    w, h, frames = 128, 72, 6
    clean = dc.pan_stream(w, h, frames, (3, -2))
    noisy = [dc.noisy(f, 4, 2000 + k) for k, f in enumerate(clean)]
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    device = [ctx.frame_from(f) for f in noisy]
    pong = [ctx.create_frame(w, h), ctx.create_frame(w, h)]
    mv, record, truth = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2), ctx.create_diff_record(), ctx.frame_from(clean[-1])
    try:
        prev_dev, prev_host = device[0], noisy[0]
        for k in range(1, frames):
            out = pong[k % 2]
            ctx.motion(prev_dev, device[k], mv)
            ctx.denoise_temporal(device[k], [prev_dev], [mv], out, 1, 32, 192, 255)
            vectors = ctx.download(mv)
            want = dm.denoise(noisy[k], [prev_host], [vectors], 1, 32, 192, 255)
            got = ctx.download(out)
            assert (got == want).all(), f"step {k}: {first_bad(got, want)}"
            prev_dev, prev_host = out, got
        inner = vectors[8:-8, 8:-8].reshape(-1, 2)
        assert (inner == (-3, 2)).mean() > 0.9, "lfg_motion did not find the pan: the step above tested nothing"
        before, after = sse(ctx, device[-1], truth, record), sse(ctx, prev_dev, truth, record)
        print(f"squared error against the clean frame: {before} in, {after} out ({after / before:.3f})")
        assert after < before
    finally:
        ctx.set_semantics(capi.SEMANTICS_REFERENCE)
        for f in device + pong + [mv, record, truth]:
            ctx.destroy_frame(f)
