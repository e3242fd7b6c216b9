"""lfg_upscale_edge on the GPU, byte for byte against the CPU model (tests/edge_model.py) run on the library's own tables: the
smallest shapes at which each path can break -- every read clamped, ragged tiles, both sides of the 64-column tile, equal axes --
on 0 / 255 noise, random bytes and a diagonal edge; what the definition promises, on the GPU's own output; padded pitches and
views; one launch under LFG_STAGE_SCALE; three lanes; argument checks; and one 1080p -> 4K call on eight regions of interest."""
import ctypes
import functools

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import edge_model as em
from tests.gpu_kit import ctx, first_bad, pitched, three_lanes

pytestmark = pytest.mark.gpu

SENTINEL = em.SENTINEL
SHAPES = [(1, 1, 4, 3), (5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (40, 9, 130, 20), (67, 9, 130, 20), (2, 2, 131, 67), (33, 5, 65, 9),
          (24, 16, 48, 16), (24, 16, 24, 32), (24, 16, 24, 16)]


@functools.lru_cache(maxsize=None)
def positions(n_in, n_out):
    return capi.upscale_edge_positions(n_in, n_out)


@functools.lru_cache(maxsize=None)
def shapes():
    return capi.upscale_edge_shapes()


def model(frame, ow, oh, roi=None):
    h, w = frame.shape[:2]
    return em.upscale(frame, ow, oh, positions(w, ow), positions(h, oh), shapes(), roi=roi)


def inputs(w, h):
    return (("noise", em.binary_noise(w, h, 100 * w + h)), ("bytes", em.random_bytes(w, h, 200 * w + h)), ("edge", em.diagonal_edge(w, h)))


def gpu(ctx, frame, ow, oh):
    f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
    try:
        ctx.upscale_edge(f, o)
        return ctx.download(o)
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


# ---- 1. bytes equal the model

@pytest.mark.parametrize("shape", SHAPES, ids=["{}x{}-{}x{}".format(*s) for s in SHAPES])
def test_equals_the_model(ctx, shape):
    w, h, ow, oh = shape
    for name, frame in inputs(w, h):
        got, want = gpu(ctx, frame, ow, oh), model(frame, ow, oh)
        assert (got == want).all(), f"{w}x{h}->{ow}x{oh} {name}: {first_bad(got, want)}"


def test_a_quarter_of_1080p_equals_the_model(ctx):
    frame = em.binary_noise(480, 270, 9)
    frame[60:200, 100:380] = em.diagonal_edge(280, 140)
    got, want = gpu(ctx, frame, 960, 540), model(frame, 960, 540)
    assert (got == want).all(), first_bad(got, want)


def test_1080p_to_4k_on_eight_regions(ctx):
    w, h, ow, oh, n = 1920, 1080, 3840, 2160, 64
    frame = em.binary_noise(w, h, 4)
    frame[300:800, 500:1500] = em.diagonal_edge(1000, 500)
    got = gpu(ctx, frame, ow, oh)
    rng = np.random.default_rng(12)
    regions = [(0, 0), (ow - n, 0), (0, oh - n), (ow - n, oh - n), (2000 - n // 2, 1100)]
    regions += [(int(rng.integers(0, ow - n)), int(rng.integers(0, oh - n))) for _ in range(3)]
    for x0, y0 in regions:
        want = model(frame, ow, oh, roi=(x0, y0, n, n))
        assert (got[y0:y0 + n, x0:x0 + n] == want).all(), f"region at {x0}, {y0}: {first_bad(got[y0:y0 + n, x0:x0 + n], want)}"


# ---- 2. what the definition promises, on the GPU's own output

@pytest.mark.parametrize("shape", [(13, 7, 26, 14), (40, 9, 130, 20), (2, 2, 131, 67), (24, 16, 24, 16)], ids=["2x", "ragged", "one-bracket", "equal"])
def test_constants_stay_and_outputs_lie_within_their_bracket(ctx, shape):
    w, h, ow, oh = shape
    for value in (0, 129, 255):
        assert (gpu(ctx, np.full((h, w, 4), value, np.uint8), ow, oh) == value).all(), value
    for name, frame in inputs(w, h):
        got, (lo, hi) = gpu(ctx, frame, ow, oh), em.bracket(frame, ow, oh)
        assert (got >= lo).all() and (got <= hi).all(), name


def test_differs_from_lanczos3_on_the_edge_frame(ctx):
    frame = em.diagonal_edge(40, 24)
    f, o = ctx.frame_from(frame), ctx.create_frame(80, 48)
    try:
        ctx.resample(f, o, capi.FILTER_LANCZOS3)
        separable = ctx.download(o)
        ctx.upscale_edge(f, o)
        got = ctx.download(o)
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)
    assert (got != separable).any(-1).mean() > 0.02
    assert got.min() >= 40 and got.max() <= 200 and (separable.min() < 40 or separable.max() > 200)      # the one that rings is Lanczos


# ---- 3. padded pitches and views

def test_padded_pitches_keep_their_padding(ctx):
    for (w, h, ow, oh), pad_in, pad_out in (((33, 5, 65, 9), 3, 5), ((13, 7, 26, 14), 1, 7), ((24, 16, 24, 32), 2, 1)):
        frame = em.random_bytes(w, h, 11 * w + h)
        big_in, src = pitched(ctx, frame, pad_in)
        big_out, dst = pitched(ctx, np.full((oh, ow, 4), SENTINEL, np.uint8), pad_out)
        try:
            ctx.upscale_edge(src, dst)
            got, kept = ctx.download(big_out), ctx.download(big_in)
            want = model(frame, ow, oh)
            assert (got[:, :ow] == want).all(), first_bad(got[:, :ow], want)
            assert (got[:, ow:] == SENTINEL).all(), "the output's padding was written"
            assert (kept[:, :w] == frame).all() and (kept[:, w:] == SENTINEL).all()
        finally:
            ctx.destroy_frame(big_in)
            ctx.destroy_frame(big_out)


def test_a_view_is_its_own_image(ctx):
    big_w, big_h, w, h, x0, y0, ow, oh = 40, 12, 13, 7, 3, 2, 29, 15
    inside = em.random_bytes(w, h, 77)
    results = []
    for outside in (0xFF, 0x00):
        big = np.full((big_h, big_w, 4), outside, np.uint8)
        big[y0:y0 + h, x0:x0 + w] = inside
        src, dst = ctx.frame_from(big), ctx.frame_from(np.full((big_h + oh, big_w, 4), SENTINEL, np.uint8))
        try:
            view_in = capi.Context.wrap(src.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
            view_out = capi.Context.wrap(dst.data + (y0 * big_w + x0) * 4, ow, oh, pitch=big_w * 4)
            ctx.upscale_edge(view_in, view_out)
            got = ctx.download(dst)
            results.append(got[y0:y0 + oh, x0:x0 + ow].copy())
            got[y0:y0 + oh, x0:x0 + ow] = SENTINEL
            assert (got == SENTINEL).all() and (ctx.download(src) == big).all()
        finally:
            ctx.destroy_frame(src)
            ctx.destroy_frame(dst)
    assert (results[0] == results[1]).all() and (results[0] == model(inside, ow, oh)).all()


# ---- 4. the launch

def test_timed_as_the_scale_stage_in_one_launch(ctx):
    f, o = ctx.frame_from(em.binary_noise(13, 7, 1)), ctx.create_frame(17, 10)
    try:
        launches = ctypes.c_uint64()
        before = ctx.lib.lfg_scale_last_kernel(ctx.h)
        assert ctx.lib.lfg_profile_enable(ctx.h, 1) == 0 and ctx.lib.lfg_profile_reset(ctx.h) == 0
        ctx.upscale_edge(f, o)
        assert ctx.lib.lfg_profile_get(ctx.h, capi.STAGE_SCALE, None, ctypes.byref(launches)) == 0 and launches.value == 1
        assert ctx.lib.lfg_scale_last_kernel(ctx.h) == before
    finally:
        ctx.lib.lfg_profile_enable(ctx.h, 0)
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


def test_three_lanes_give_the_same(ctx):
    """More (in, out) pairs than the context keeps positions for (14), with no sync between the calls: a table is dropped and
    built while kernels that read others are queued on other lanes."""
    cases = [(13 + i, 7, 26 + 3 * i, 14 + i) for i in range(18)] + [(67, 9, 130, 20), (24, 16, 24, 16), (13, 7, 26, 14)]
    frames = [(em.random_bytes(w, h, 900 + i),) for i, (w, h, _, _) in enumerate(cases)]
    alone = []
    for (frame,), (w, h, ow, oh) in zip(frames, cases):
        alone.append(gpu(ctx, frame, ow, oh))
        assert (alone[-1] == model(frame, ow, oh)).all(), (w, h, ow, oh)

    def enqueue(i, frame):
        f, o = ctx.frame_from(frame), ctx.create_frame(*cases[i][2:])
        ctx.upscale_edge(f, o)
        return f, o

    three_lanes(ctx, frames, enqueue, alone)


def test_position_cache_survives_many_pairs():
    """The context keeps 14 position tables, for both axes together.  Eight calls with sixteen distinct (in, out) pairs: the
    ninth call's trim drops the first call's two, which leaves the second call's width pair the oldest entry, and the ninth
    call takes that pair for its width and a new one for its height -- whose table must not cost the width's its memory."""
    cases = [(13 + i, 5 + i, 26 + 3 * i, 11 + 2 * i) for i in range(8)]
    cases.append((cases[1][0], 23, cases[1][2], 57))
    pairs = [p for (w, h, ow, oh) in cases for p in ((w, ow), (h, oh))]
    assert len(set(pairs[:16])) == 16 and pairs[16] == pairs[2] and pairs[17] not in pairs[:16]
    with capi.Context(0) as own:
        for i, (w, h, ow, oh) in enumerate(cases):
            frame = em.random_bytes(w, h, 700 + i)
            got, want = gpu(own, frame, ow, oh), model(frame, ow, oh)
            assert (got == want).all(), f"{w}x{h}->{ow}x{oh}: {first_bad(got, want)}"


# ---- 5. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h, ow, oh = 16, 6, 24, 9
    host = em.binary_noise(w, h + 2, 5)
    big_in, good_in = pitched(ctx, host, 4)
    good_in = capi.Context.wrap(big_in.data, w, h, pitch=good_in.pitch)
    big_out, good_out = pitched(ctx, np.full((oh, ow, 4), SENTINEL, np.uint8), 4)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        def framed(like, ptr=None, width=None, height=None, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height = like.data if ptr is None else ptr, like.width if width is None else width, like.height if height is None else height
            f.pitch, f.format = pitch or like.pitch, capi.FORMAT_RGBA8
            return f

        no_data = framed(good_in)
        no_data.data = None
        invalid = [(None, B(good_in), B(good_out)), (ctx.h, None, B(good_out)), (ctx.h, B(good_in), None),
                   (ctx.h, B(no_data), B(good_out)), (ctx.h, B(good_in), B(no_data)),
                   (ctx.h, B(mv), B(good_out)), (ctx.h, B(good_in), B(mv)),                                     # MV_S8X2 on either side
                   (ctx.h, B(framed(good_in, width=0)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, height=0))),
                   (ctx.h, B(framed(good_in, ptr=good_in.data + 2)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, ptr=good_out.data + 2))),
                   (ctx.h, B(framed(good_in, pitch=good_in.pitch + 2)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, pitch=good_out.pitch + 2))),
                   (ctx.h, B(framed(good_in, pitch=w * 4 - 4)), B(good_out)), (ctx.h, B(good_in), B(framed(good_out, pitch=ow * 4 - 4))),
                   (ctx.h, B(good_in), B(good_in)),                                                             # in place
                   (ctx.h, B(good_in), B(framed(good_in, ptr=good_in.data + good_in.pitch)))]                   # out one row into in
        results = [lib.lfg_upscale_edge(*c) for c in invalid]
        assert all(rc == capi.ERR_INVALID for rc in results), results
        assert "lfg_upscale_edge" in lib.lfg_last_error(ctx.h).decode()
        shrinking = [(ctx.h, B(good_in), B(framed(good_out, width=w - 1))), (ctx.h, B(good_in), B(framed(good_out, height=h - 1))),
                     (ctx.h, B(good_in), B(framed(good_out, width=w - 1, height=h - 1)))]
        results = [lib.lfg_upscale_edge(*c) for c in shrinking]
        assert all(rc == capi.ERR_UNSUPPORTED for rc in results), results
        assert "lfg_upscale_edge" in lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert (ctx.download(big_out) == SENTINEL).all() and (ctx.download(big_in)[:, :w] == host).all()
        ctx.upscale_edge(good_in, good_out)                               # a valid call next to the bad ones works
        got = ctx.download(big_out)
        assert (got[:, :ow] == model(host[:h], ow, oh)).all() and (got[:, ow:] == SENTINEL).all()
        for filt in (6, 7):                        # and the resampler still knows no seventh filter
            assert lib.lfg_resample(ctx.h, B(good_in), B(good_out), filt) == capi.ERR_INVALID
            assert lib.lfg_resample_antiring(ctx.h, B(good_in), B(good_out), filt, 32) == capi.ERR_INVALID
    finally:
        for f in (mv, big_in, big_out):
            ctx.destroy_frame(f)
