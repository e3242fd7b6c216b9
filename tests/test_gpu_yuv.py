"""Colour conversion on the GPU: lfg_nv12_to_rgba and lfg_rgba_to_nv12 byte for byte against the CPU model (tests/yuv_model.py)
-- the smallest shapes that can go wrong under all 8 mode combinations, padded and aligned pitches with sentinels around every
row, regions of interest, every (Y, Cb, Cr) and every (R, G, B), argument checks, two lanes -- and lfg_host with raw NV12 in and
out against the chain model -> CPU scale and interpolation models -> model."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import yuv_model as ym
from tests.gpu_kit import ctx, host_run

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
SHAPES = [(2, 2), (4, 2), (16, 2), (18, 6), (62, 34), (130, 4)]
MODE_IDS = [f"{'601' if m == ym.BT601 else '709'}-{'limited' if r == ym.LIMITED else 'full'}-{'replicate' if s == ym.REPLICATE else 'left'}"
            for m, r, s in ym.MODES]
modes = pytest.mark.parametrize("mode", ym.MODES, ids=MODE_IDS)
shapes = pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])


class Plane:
    """`rows` rows of `row_bytes` bytes, `pitch` apart, `lead` bytes into device memory that is otherwise SENTINEL: a plane of
    an lfg_nv12 or the bytes of an RGBA frame.  fetch() returns the rows and asserts that no other byte has changed."""

    def __init__(self, ctx, rows, row_bytes, pitch=None, lead=0, data=None):
        self.ctx, self.rows, self.row_bytes, self.pitch, self.lead = ctx, rows, row_bytes, pitch or row_bytes, lead
        self.size = lead + (rows - 1) * self.pitch + row_bytes + 64
        texel_rows = -(-self.size // 4096)
        self.host = np.full(texel_rows * 4096, SENTINEL, np.uint8)
        if data is not None:
            self.view(self.host)[...] = np.ascontiguousarray(data).reshape(rows, row_bytes)
        self.frame = ctx.frame_from(self.host.reshape(texel_rows, 1024, 4))

    def view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.lead:], (self.rows, self.row_bytes), (self.pitch, 1))

    @property
    def ptr(self):
        return self.frame.data + self.lead

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


def nv12_of(yp, uvp, w, h):
    return capi.Nv12(yp.ptr, uvp.ptr, w, h, yp.pitch, uvp.pitch)


def rgba_of(p, w, h):
    return capi.Context.wrap(p.ptr, w, h, pitch=p.pitch)


def first_bad(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first at {bad[:3].tolist()}: got {[int(got[tuple(b)]) for b in bad[:3]]}, model {[int(want[tuple(b)]) for b in bad[:3]]}"


def check_both_directions(ctx, w, h, mode, seed, y_pitch=None, uv_pitch=None, rgba_pitch=None, leads=(0, 0, 0)):
    """Random planes -> RGBA and a random frame -> planes, at these pitches and leading offsets: the model's bytes, and every
    byte around the rows keeps its sentinel."""
    matrix, rng, siting = mode
    y, uv = ym.random_nv12(w, h, seed)
    rgba = ym.random_rgba(w, h, seed + 1)
    planes = []
    try:
        yp = Plane(ctx, h, w, y_pitch, leads[0], y)
        uvp = Plane(ctx, h // 2, w, uv_pitch, leads[1], uv)
        out = Plane(ctx, h, w * 4, rgba_pitch, leads[2])
        planes += [yp, uvp, out]
        ctx.nv12_to_rgba(nv12_of(yp, uvp, w, h), rgba_of(out, w, h), matrix, rng, siting)
        got, want = out.fetch("rgba").reshape(h, w, 4), ym.nv12_to_rgba(y, uv, matrix, rng, siting)
        assert (got == want).all(), f"NV12 -> RGBA {w}x{h}: {first_bad(got, want)}"
        assert yp.unchanged() and uvp.unchanged()

        check_to_nv12(ctx, rgba, mode, y_pitch, uv_pitch, rgba_pitch, leads)
    finally:
        for p in planes:
            p.free()


def check_to_nv12(ctx, rgba, mode, y_pitch=None, uv_pitch=None, rgba_pitch=None, leads=(0, 0, 0)):
    """`rgba` -> planes at these pitches and leading offsets: the model's bytes, sentinels kept.  Returns (y, uv) as the GPU wrote them."""
    (h, w), planes = rgba.shape[:2], []
    try:
        src = Plane(ctx, h, w * 4, rgba_pitch, leads[2], rgba)
        yo = Plane(ctx, h, w, y_pitch, leads[0])
        uvo = Plane(ctx, h // 2, w, uv_pitch, leads[1])
        planes += [src, yo, uvo]
        ctx.rgba_to_nv12(rgba_of(src, w, h), nv12_of(yo, uvo, w, h), *mode)
        want_y, want_uv = ym.rgba_to_nv12(rgba, *mode)
        got_y, got_uv = yo.fetch("y"), uvo.fetch("uv").reshape(h // 2, w // 2, 2)
        assert (got_y == want_y).all(), f"RGBA -> NV12 luma {w}x{h}: {first_bad(got_y, want_y)}"
        assert (got_uv == want_uv).all(), f"RGBA -> NV12 chroma {w}x{h}: {first_bad(got_uv, want_uv)}"
        assert src.unchanged()
        return got_y, got_uv
    finally:
        for p in planes:
            p.free()


# ---- 1. the smallest shapes that can go wrong, all 8 modes, both directions

@modes
@shapes
def test_equals_the_model(ctx, w, h, mode):
    check_both_directions(ctx, w, h, mode, 100 * w + h)


# ---- 2. pitches.  Padded: nothing is aligned, every item is one quad.  Aligned: the 8 x 2 items, with 0 .. 3 quads behind them

@pytest.mark.parametrize("rgba_pad", [4, 16])
@modes
@shapes
def test_padded_pitches(ctx, w, h, mode, rgba_pad):
    check_both_directions(ctx, w, h, mode, 200 * w + h, y_pitch=w + 2, uv_pitch=w + 6, rgba_pitch=w * 4 + rgba_pad)


ALIGNED_SHAPES = [(16, 2), (18, 6), (62, 34), (130, 4), (8, 2), (10, 2), (520, 6), (1030, 10)]


@modes
@pytest.mark.parametrize("w,h", ALIGNED_SHAPES, ids=[f"{w}x{h}" for w, h in ALIGNED_SHAPES])
def test_aligned_pitches_take_the_wide_items(ctx, w, h, mode):
    """Bases and pitches that allow the 8-byte and 16-byte accesses, at widths that leave 0, 1, 2 and 3 quads behind the last
    8 x 2 item, one and several waves to a row pair, one and several workgroups down the frame."""
    y_pitch, rgba_pitch = (w + 7) // 8 * 8 + 8, (w * 4 + 15) // 16 * 16 + 16
    check_both_directions(ctx, w, h, mode, 300 * w + h, y_pitch=y_pitch, uv_pitch=y_pitch + 8, rgba_pitch=rgba_pitch, leads=(8, 16, 32))


@modes
def test_one_misaligned_plane_is_enough_for_the_narrow_items(ctx, mode):
    w, h = 24, 6
    for leads, pitches in [((1, 0, 0), (24, 24, 96)), ((0, 2, 0), (24, 24, 96)), ((0, 0, 4), (24, 24, 96)), ((0, 0, 0), (28, 24, 96)),
                           ((0, 0, 0), (24, 26, 96)), ((0, 0, 0), (24, 24, 104)), ((0, 0, 0), (25, 24, 96)), ((1, 0, 0), (27, 30, 100))]:
        check_both_directions(ctx, w, h, mode, 7, y_pitch=pitches[0], uv_pitch=pitches[1], rgba_pitch=pitches[2], leads=leads)


# ---- 3. a region of interest through offset pointers

@modes
@pytest.mark.parametrize("x0,y0,w,h", [(6, 4, 18, 6), (8, 4, 24, 8), (16, 2, 42, 10)], ids=["unaligned", "aligned", "aligned-tail"])
def test_region_of_interest(ctx, mode, x0, y0, w, h):
    matrix, rng, siting = mode
    big_w, big_h = 64, 40
    y, uv = ym.random_nv12(big_w, big_h, 41)
    rgba = ym.random_rgba(big_w, big_h, 42)
    yp, uvp, fp = Plane(ctx, big_h, big_w, data=y), Plane(ctx, big_h // 2, big_w, data=uv), Plane(ctx, big_h, big_w * 4, data=rgba)
    try:
        def window(planes_y, planes_uv):
            return capi.Nv12(planes_y.ptr + y0 * big_w + x0, planes_uv.ptr + (y0 // 2) * big_w + x0, w, h, big_w, big_w)
        frame = capi.Context.wrap(fp.ptr + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
        # into the window of the frame: the rest of the frame stays
        ctx.nv12_to_rgba(window(yp, uvp), frame, matrix, rng, siting)
        want = rgba.copy()
        want[y0:y0 + h, x0:x0 + w] = ym.nv12_to_rgba(y[y0:y0 + h, x0:x0 + w], uv[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], matrix, rng, siting)
        got = fp.fetch("frame").reshape(big_h, big_w, 4)
        assert (got == want).all(), first_bad(got, want)
        assert yp.unchanged() and uvp.unchanged()
        # and from the window of the (converted) frame into the window of the planes
        ctx.rgba_to_nv12(frame, window(yp, uvp), matrix, rng, siting)
        wy, wuv = ym.rgba_to_nv12(want[y0:y0 + h, x0:x0 + w], matrix, rng, siting)
        want_y, want_uv = y.copy(), uv.copy()
        want_y[y0:y0 + h, x0:x0 + w], want_uv[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2] = wy, wuv
        got_y, got_uv = yp.fetch("y"), uvp.fetch("uv").reshape(big_h // 2, big_w // 2, 2)
        assert (got_y == want_y).all(), first_bad(got_y, want_y)
        assert (got_uv == want_uv).all(), first_bad(got_uv, want_uv)
    finally:
        for p in (yp, uvp, fp):
            p.free()


# ---- 4. every input

def test_every_yuv_triple(ctx):
    y, uv = ym.every_yuv_triple()
    f, planes = ctx.nv12_from(y, uv)
    out = ctx.create_frame(4096, 4096)
    try:
        ctx.nv12_to_rgba(planes, out, ym.BT709, ym.LIMITED, ym.REPLICATE)
        got, want = ctx.download(out), ym.nv12_to_rgba(y, uv, ym.BT709, ym.LIMITED, ym.REPLICATE)
        assert (got == want).all(), first_bad(got, want)
        for c in range(3):                                    # both clamps of every channel fired
            assert got[..., c].min() == 0 and got[..., c].max() == 255
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(out)


def test_every_rgb_triple(ctx):
    rgba = ym.every_rgb_triple()
    src = ctx.frame_from(rgba)
    f, planes = ctx.create_nv12(4096, 4096)
    try:
        ctx.rgba_to_nv12(src, planes, ym.BT601, ym.FULL, ym.REPLICATE)
        (got_y, got_uv), (want_y, want_uv) = ctx.download_nv12(f), ym.rgba_to_nv12(rgba, ym.BT601, ym.FULL, ym.REPLICATE)
        assert (got_y == want_y).all(), first_bad(got_y, want_y)
        assert (got_uv == want_uv).all(), first_bad(got_uv, want_uv)
        assert got_y.min() == 0 and got_y.max() == 255
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(src)


SATURATED_SHAPES = [(2, 2), (18, 6), (24, 4)]


@pytest.mark.parametrize("matrix", ym.MATRICES, ids=["601", "709"])
@pytest.mark.parametrize("siting", ym.SITINGS, ids=["replicate", "left"])
@pytest.mark.parametrize("w,h", SATURATED_SHAPES, ids=[f"{w}x{h}" for w, h in SATURATED_SHAPES])
def test_saturated_blue_and_red_reach_the_upper_chroma_clamp(ctx, w, h, siting, matrix):
    """The one clamp of RGBA -> NV12 that can fire: uniform quads of pure blue and pure red under the full range give 128 + 128
    (no quad of every_rgb_triple is uniform, and random bytes come nowhere near).  Without the clamp the pair word would carry
    256 into its other byte.  Through the one-quad items (tight and odd pitches) and the 8 x 2 items with their tail."""
    mode = (matrix, ym.FULL, siting)
    aligned = dict(y_pitch=(w + 7) // 8 * 8 + 8, uv_pitch=(w + 7) // 8 * 8 + 16, rgba_pitch=(w * 4 + 15) // 16 * 16 + 16, leads=(8, 16, 32))
    for layout in ({}, dict(y_pitch=w + 1, uv_pitch=w + 6, rgba_pitch=w * 4 + 4), aligned):
        blue, red = ym.saturated_rgba(w, h, 900 + w)
        _, uv = check_to_nv12(ctx, blue, mode, **layout)
        assert (uv[0, :, 0] == 255).all() and (uv[0, :, 1] < 128).all(), uv[0]
        _, uv = check_to_nv12(ctx, red, mode, **layout)
        assert (uv[0, :, 1] == 255).all() and (uv[0, :, 0] < 128).all(), uv[0]


# ---- 5. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 16, 6
    y, uv = ym.random_nv12(w, h, 5)
    rgba = ym.random_rgba(w, h, 6)
    yp, uvp, fp = Plane(ctx, h, w, w + 8, data=y), Plane(ctx, h // 2, w, w + 8, data=uv), Plane(ctx, h, w * 4, w * 4 + 16, data=rgba)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        good, frame = nv12_of(yp, uvp, w, h), rgba_of(fp, w, h)

        def planes(**change):
            p = capi.Nv12(good.y, good.uv, good.width, good.height, good.y_pitch, good.uv_pitch)
            for name, value in change.items():
                setattr(p, name, value)
            return p

        def framed(ptr=None, width=w, height=h, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height, f.pitch, f.format = ptr or frame.data, width, height, pitch or frame.pitch, capi.FORMAT_RGBA8
            return f

        bad_planes = [planes(y=None), planes(uv=None), planes(width=w - 1), planes(height=h - 1), planes(width=w + 2), planes(height=h + 2),
                      planes(width=0), planes(height=0), planes(y_pitch=w - 1), planes(uv_pitch=w - 2), planes(uv_pitch=w + 1),
                      planes(uv=good.uv + 1),
                      planes(y=frame.data + 8), planes(uv=frame.data + 8),                    # a plane inside the frame
                      planes(y=frame.data - w, y_pitch=w)]                                   # its last row reaches the frame
        bad_frames = [framed(width=w - 2), framed(height=h - 2), framed(pitch=w * 4 + 2), framed(ptr=frame.data + 2), capi.Frame(), mv]
        both = (lib.lfg_nv12_to_rgba, lambda p, f: (B(p), B(f))), (lib.lfg_rgba_to_nv12, lambda p, f: (B(f), B(p)))
        results = []
        for call, order in both:
            results += [call(ctx.h, *order(p, frame), 0, 0, 0) for p in bad_planes]
            results += [call(ctx.h, *order(good, f), 0, 0, 0) for f in bad_frames]
            results += [call(ctx.h, *order(good, frame), *m) for m in [(2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)]]
            results += [call(None, *order(good, frame), 0, 0, 0)]
        results += [lib.lfg_nv12_to_rgba(ctx.h, None, B(frame), 0, 0, 0), lib.lfg_nv12_to_rgba(ctx.h, B(good), None, 0, 0, 0),
                    lib.lfg_rgba_to_nv12(ctx.h, None, B(good), 0, 0, 0), lib.lfg_rgba_to_nv12(ctx.h, B(frame), None, 0, 0, 0)]
        # the planes of an output may not overlap each other (as inputs they may)
        results += [lib.lfg_rgba_to_nv12(ctx.h, B(frame), B(planes(uv=good.y + 2 * good.y_pitch)), 0, 0, 0)]
        assert all(rc == -1 for rc in results), results           # LFG_ERR_INVALID
        assert lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert yp.unchanged() and uvp.unchanged() and fp.unchanged()
        # a valid call next to the bad ones works; as inputs the planes may overlap
        overlapping = planes(uv=good.y + 2 * good.y_pitch)
        ctx.nv12_to_rgba(overlapping, frame, ym.BT709, ym.FULL, ym.LEFT)
        pairs = np.stack([y[2:2 + h // 2, 0::2], y[2:2 + h // 2, 1::2]], axis=-1)
        want = ym.nv12_to_rgba(y, pairs, ym.BT709, ym.FULL, ym.LEFT)
        got = fp.fetch("frame").reshape(h, w, 4)
        assert (got == want).all(), first_bad(got, want)
    finally:
        ctx.destroy_frame(mv)
        for p in (yp, uvp, fp):
            p.free()


# ---- 6. two lanes

def test_two_lanes_give_the_same(ctx):
    jobs = [((62, 34), ym.MODES[3]), ((130, 4), ym.MODES[6]), ((16, 2), ym.MODES[1]), ((520, 6), ym.MODES[7])]
    ctx.lanes(2)
    made = []
    try:
        for i, ((w, h), (matrix, rng, siting)) in enumerate(jobs):
            ctx.lane_select(i % 2)
            y, uv = ym.random_nv12(w, h, 60 + i)
            f, planes = ctx.nv12_from(y, uv)
            mid = ctx.create_frame(w, h)
            g, back = ctx.create_nv12(w, h)
            ctx.nv12_to_rgba(planes, mid, matrix, rng, siting)     # both on the lane, in order: no wait in between
            ctx.rgba_to_nv12(mid, back, matrix, rng, siting)
            made.append((f, mid, g, y, uv, (matrix, rng, siting)))
        ctx.sync()
        for f, mid, g, y, uv, mode in made:
            want = ym.nv12_to_rgba(y, uv, *mode)
            assert (ctx.download(mid) == want).all()
            want_y, want_uv = ym.rgba_to_nv12(want, *mode)
            got_y, got_uv = ctx.download_nv12(g)
            assert (got_y == want_y).all() and (got_uv == want_uv).all()
    finally:
        for f, mid, g, *_ in made:
            for x in (f, mid, g):
                ctx.destroy_frame(x)
        ctx.lane_select(0)
        ctx.lanes(1)


# ---- 7. lfg_host with raw NV12 in and out

@pytest.mark.parametrize("options,mode", [((), (ym.BT709, ym.LIMITED, ym.LEFT)),
                                          (("--yuv-matrix", "601", "--yuv-range", "full", "--chroma", "replicate"), (ym.BT601, ym.FULL, ym.REPLICATE))],
                         ids=["defaults", "601-full-replicate"])
def test_host_nv12_in_and_out(ctx, oracle, tmp_path, options, mode):
    """64 x 36 -> 128 x 72, three frames: model (NV12 -> RGBA), the CPU scale model (+-1 LSB, so the real frames are taken from
    what the device shows: its NV12 output is the model's conversion of a frame within 1 LSB of the scale model), motion and
    interpolation models on the device's own upscaled frames, model (RGBA -> NV12)."""
    from linux_fg_amd import synth
    w, h, n = 64, 36, 3
    rgba = [synth.make_prev(w, h, synth.BASE_SEED)]
    for k in range(1, n):
        rgba.append(synth.translate(rgba[-1], (3, -2), synth.BASE_SEED + k))
    nv12 = [ym.rgba_to_nv12(f, *mode) for f in rgba]
    info, shown = host_run(tmp_path / "nv12", nv12, (2 * w, 2 * h), "--input-format", "nv12", "--output-format", "nv12", *options)
    assert info["presented"] == 2 * n - 1 and info["input_format"] == "nv12" and info["output_format"] == "nv12"
    # the same stream with RGBA out: the frames the NV12 sink converted
    report, frames = host_run(tmp_path / "rgba", nv12, (2 * w, 2 * h), "--input-format", "nv12", *options)
    assert report["input_format"] == "nv12" and report["output_format"] == "rgba" and len(frames) == 2 * n - 1
    for k in range(n):                                        # real frames: the converted input, upscaled
        want = oracle.scale(ym.nv12_to_rgba(*nv12[k], *mode), 2 * w, 2 * h)
        assert np.abs(frames[2 * k].astype(np.int16) - want.astype(np.int16)).max() <= 1, k
    for k in range(n - 1):                                    # generated frames: exact, from the device's own upscaled frames
        prev_up, curr_up = frames[2 * k], frames[2 * k + 2]
        mv = oracle.motion(prev_up, curr_up, 8, 16.0)
        assert (frames[2 * k + 1] == oracle.interpolate(prev_up, curr_up, mv, 0.5)).all(), k
    for k, (got_y, got_uv) in enumerate(shown):               # the sink: the model's conversion of each presented frame
        want_y, want_uv = ym.rgba_to_nv12(frames[k], *mode)
        assert (got_y == want_y).all() and (got_uv == want_uv).all(), k
