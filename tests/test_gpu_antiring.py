"""lfg_resample_antiring on the GPU, byte for byte against the CPU model (tests/antiring_model.py) run on the library's own
tables: the smallest shapes at which each path can break -- both axes growing, one, none, across the 64-column tile -- under
three strengths and the five filters that can ring; what the definition promises, on the GPU's own output; padded pitches and
views; argument checks; three lanes; and one 1080p -> 4K call on eight regions of interest."""
import ctypes
import functools

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import antiring_model as am
from tests import resample_model as rm
from tests.gpu_kit import ctx, first_bad, pitched, three_lanes

pytestmark = pytest.mark.gpu

SENTINEL = rm.SENTINEL
BOTH_GROW = [(5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (40, 9, 130, 20), (2, 2, 131, 67), (1, 1, 4, 3), (33, 5, 65, 9), (67, 9, 130, 20),
             (64, 36, 128, 72)]
ONE_GROWS = [am.HORIZONTAL_ONLY, am.VERTICAL_ONLY]
NONE_GROWS = [(24, 16, 24, 16), (37, 19, 12, 6)]
RINGING = tuple(f for f in rm.FILTERS if f != rm.NEAREST)
STRENGTHS = (1, 24, 64)


@functools.lru_cache(maxsize=None)
def taps(filt, n_in, n_out):
    return capi.resample_taps(filt, n_in, n_out)


def model(frame, ow, oh, filt, strength, roi=None):
    h, w = frame.shape[:2]
    return am.antiring(frame, ow, oh, filt, strength, taps(filt, w, ow), taps(filt, h, oh), roi=roi)


def random_bytes(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def gpu(ctx, frame, ow, oh, filt, strength=None):
    """lfg_resample_antiring of `frame`, or lfg_resample with strength=None, through tight frames."""
    f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
    try:
        if strength is None:
            ctx.resample(f, o, filt)
        else:
            ctx.resample_antiring(f, o, filt, strength)
        return ctx.download(o)
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


def ids(shapes):
    return ["{}x{}-{}x{}".format(*s) for s in shapes]


# ---- 1. bytes equal the model

@pytest.mark.parametrize("shape", BOTH_GROW + ONE_GROWS, ids=ids(BOTH_GROW + ONE_GROWS))
def test_equals_the_model(ctx, shape):
    w, h, ow, oh = shape
    noise, rand = rm.binary_noise(w, h, 100 * w + h), random_bytes(w, h, 200 * w + h)
    f, g, o = ctx.frame_from(noise), ctx.frame_from(rand), ctx.create_frame(ow, oh)
    try:
        for filt in RINGING:
            for frame, src, strengths in ((noise, f, STRENGTHS), (rand, g, (64, 33))):
                for s in strengths:
                    ctx.resample_antiring(src, o, filt, s)
                    got, want = ctx.download(o), model(frame, ow, oh, filt, s)
                    assert (got == want).all(), f"{w}x{h}->{ow}x{oh} {rm.NAMES[filt]} S {s}: {first_bad(got, want)}"
    finally:
        for frame in (f, g, o):
            ctx.destroy_frame(frame)


def test_a_quarter_of_1080p_equals_the_model(ctx):
    frame = rm.binary_noise(480, 270, 9)
    got, want = gpu(ctx, frame, 960, 540, rm.LANCZOS3, 24), model(frame, 960, 540, rm.LANCZOS3, 24)
    assert (got == want).all(), first_bad(got, want)


# ---- 2. where it is lfg_resample, and what the definition promises

def test_strength_zero_nearest_and_no_growing_axis_are_resample(ctx):
    for w, h, ow, oh in NONE_GROWS:
        frame = rm.binary_noise(w, h, 3 * w + h)
        for filt in rm.FILTERS:
            want = gpu(ctx, frame, ow, oh, filt)
            for s in (0, 1, 64):
                assert (gpu(ctx, frame, ow, oh, filt, s) == want).all(), (w, h, ow, oh, rm.NAMES[filt], s)
    for w, h, ow, oh in [(13, 7, 26, 14), (13, 7, 17, 10)] + ONE_GROWS:
        frame = rm.binary_noise(w, h, 5 * w + h)
        for filt in rm.FILTERS:
            want = gpu(ctx, frame, ow, oh, filt)
            assert (gpu(ctx, frame, ow, oh, filt, 0) == want).all(), (w, h, ow, oh, rm.NAMES[filt])
            if filt in (rm.NEAREST, rm.BILINEAR):                     # one tap; a convex combination of the bracket
                for s in STRENGTHS:
                    assert (gpu(ctx, frame, ow, oh, filt, s) == want).all(), (w, h, ow, oh, rm.NAMES[filt], s)
    frame = rm.binary_noise(13, 7, 72)                                # and where it is not: the clamp binds on most pixels
    differ = (gpu(ctx, frame, 26, 14, rm.LANCZOS3, 64) != gpu(ctx, frame, 26, 14, rm.LANCZOS3)).any(-1).mean()
    assert differ >= 0.5, differ


@pytest.mark.parametrize("shape", [(13, 7, 26, 14), (40, 9, 130, 20), (2, 2, 131, 67)], ids=ids([(13, 7, 26, 14), (40, 9, 130, 20), (2, 2, 131, 67)]))
def test_full_strength_stays_within_the_four_texels(ctx, shape):
    w, h, ow, oh = shape
    (ax, bx), (ay, by) = am.brackets(w, ow), am.brackets(h, oh)
    for frame in (rm.binary_noise(w, h, 7 * w + h), random_bytes(w, h, 8 * w + h)):
        corners = np.stack([frame[ay][:, ax], frame[ay][:, bx], frame[by][:, ax], frame[by][:, bx]])
        for filt in RINGING:
            got = gpu(ctx, frame, ow, oh, filt, 64)
            assert (got >= corners.min(0)).all() and (got <= corners.max(0)).all(), rm.NAMES[filt]
    for value in (0, 129, 255):                                       # a constant frame stays constant
        assert (gpu(ctx, np.full((h, w, 4), value, np.uint8), ow, oh, rm.LANCZOS3, 40) == value).all()


def test_timed_as_the_scale_stage_in_one_launch(ctx):
    f, o = ctx.frame_from(rm.binary_noise(13, 7, 1)), ctx.create_frame(17, 10)
    try:
        launches = ctypes.c_uint64()
        assert ctx.lib.lfg_profile_enable(ctx.h, 1) == 0 and ctx.lib.lfg_profile_reset(ctx.h) == 0
        ctx.resample_antiring(f, o, capi.FILTER_LANCZOS3, 64)
        assert ctx.lib.lfg_profile_get(ctx.h, capi.STAGE_SCALE, None, ctypes.byref(launches)) == 0 and launches.value == 1
    finally:
        ctx.lib.lfg_profile_enable(ctx.h, 0)
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


# ---- 3. padded pitches and views

def test_padded_pitches_keep_their_padding(ctx):
    for (w, h, ow, oh), pad_in, pad_out in (((33, 5, 65, 9), 3, 5), ((13, 7, 26, 14), 1, 7), (am.VERTICAL_ONLY, 2, 1)):
        frame = rm.binary_noise(w, h, 11 * w + h)
        big_in, src = pitched(ctx, frame, pad_in)
        big_out, dst = pitched(ctx, np.full((oh, ow, 4), SENTINEL, np.uint8), pad_out)
        try:
            ctx.resample_antiring(src, dst, capi.FILTER_LANCZOS3, 48)
            got, kept = ctx.download(big_out), ctx.download(big_in)
            want = model(frame, ow, oh, rm.LANCZOS3, 48)
            assert (got[:, :ow] == want).all(), first_bad(got[:, :ow], want)
            assert (got[:, ow:] == SENTINEL).all(), "the output's padding was written"
            assert (kept[:, :w] == frame).all() and (kept[:, w:] == SENTINEL).all()
        finally:
            ctx.destroy_frame(big_in)
            ctx.destroy_frame(big_out)


def test_a_view_is_its_own_image(ctx):
    big_w, big_h, w, h, x0, y0, ow, oh = 40, 12, 13, 7, 3, 2, 29, 15
    inside = rm.binary_noise(w, h, 77)
    results = []
    for outside in (0xFF, 0x00):
        big = np.full((big_h, big_w, 4), outside, np.uint8)
        big[y0:y0 + h, x0:x0 + w] = inside
        src, dst = ctx.frame_from(big), ctx.frame_from(np.full((big_h + oh, big_w, 4), SENTINEL, np.uint8))
        try:
            view_in = capi.Context.wrap(src.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
            view_out = capi.Context.wrap(dst.data + (y0 * big_w + x0) * 4, ow, oh, pitch=big_w * 4)
            ctx.resample_antiring(view_in, view_out, capi.FILTER_LANCZOS3, 64)
            got = ctx.download(dst)
            results.append(got[y0:y0 + oh, x0:x0 + ow].copy())
            got[y0:y0 + oh, x0:x0 + ow] = SENTINEL
            assert (got == SENTINEL).all() and (ctx.download(src) == big).all()
        finally:
            ctx.destroy_frame(src)
            ctx.destroy_frame(dst)
    assert (results[0] == results[1]).all() and (results[0] == model(inside, ow, oh, rm.LANCZOS3, 64)).all()


# ---- 4. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h, ow, oh = 16, 6, 24, 9
    host = rm.binary_noise(w, h + 2, 5)
    big_in, good_in = pitched(ctx, host, 4)
    good_in = capi.Context.wrap(big_in.data, w, h, pitch=good_in.pitch)
    big_out, good_out = pitched(ctx, np.full((oh, ow, 4), SENTINEL, np.uint8), 4)
    tall = ctx.frame_from(rm.binary_noise(w, 200, 6))                 # 200 -> 5 rows: more than 64 taps under Lanczos-3
    short_out = capi.Context.wrap(big_out.data, ow, 5, pitch=good_out.pitch)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    F, S = capi.FILTER_CATMULL_ROM, 32
    try:
        def framed(like, ptr=None, width=None, height=None, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height = like.data if ptr is None else ptr, like.width if width is None else width, like.height if height is None else height
            f.pitch, f.format = pitch or like.pitch, capi.FORMAT_RGBA8
            return f

        no_data = framed(good_in)
        no_data.data = None
        calls = [(ctx.h, B(good_in), B(good_out), F, -1), (ctx.h, B(good_in), B(good_out), F, 65), (ctx.h, B(good_in), B(good_out), F, 1000),
                 (ctx.h, B(good_in), B(good_out), capi.FILTER_NEAREST, 65),                                    # ... also where no pass would qualify
                 (None, B(good_in), B(good_out), F, S), (ctx.h, None, B(good_out), F, S), (ctx.h, B(good_in), None, F, S),
                 (ctx.h, B(no_data), B(good_out), F, S), (ctx.h, B(good_in), B(no_data), F, S),
                 (ctx.h, B(mv), B(good_out), F, S), (ctx.h, B(good_in), B(mv), F, S),                          # MV_S8X2 on either side
                 (ctx.h, B(framed(good_in, width=0)), B(good_out), F, S), (ctx.h, B(good_in), B(framed(good_out, height=0)), F, S),
                 (ctx.h, B(framed(good_in, ptr=good_in.data + 2)), B(good_out), F, S), (ctx.h, B(good_in), B(framed(good_out, ptr=good_out.data + 2)), F, S),
                 (ctx.h, B(framed(good_in, pitch=good_in.pitch + 2)), B(good_out), F, S), (ctx.h, B(good_in), B(framed(good_out, pitch=good_out.pitch + 2)), F, S),
                 (ctx.h, B(framed(good_in, pitch=w * 4 - 4)), B(good_out), F, S), (ctx.h, B(good_in), B(framed(good_out, pitch=ow * 4 - 4)), F, S),
                 (ctx.h, B(good_in), B(good_in), F, S),                                                        # in place
                 (ctx.h, B(good_in), B(framed(good_in, ptr=good_in.data + good_in.pitch)), F, S),              # out one row into in
                 (ctx.h, B(good_in), B(good_out), -1, S), (ctx.h, B(good_in), B(good_out), 6, S)]              # unknown filters
        results = [lib.lfg_resample_antiring(*c) for c in calls]
        assert all(rc == capi.ERR_INVALID for rc in results), results
        assert "lfg_resample_antiring" in lib.lfg_last_error(ctx.h).decode()
        assert lib.lfg_resample_antiring(ctx.h, B(tall), B(short_out), capi.FILTER_LANCZOS3, S) == capi.ERR_UNSUPPORTED   # a refused table
        assert lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert (ctx.download(big_out) == SENTINEL).all() and (ctx.download(big_in)[:, :w] == host).all()
        ctx.resample(good_in, good_out, F)                            # a valid call next to the bad ones works, plain and anti-ringed
        want = rm.resample_int(host[:h], taps(F, w, ow), taps(F, h, oh))
        assert (ctx.download(big_out)[:, :ow] == want).all()
        ctx.resample_antiring(good_in, good_out, F, S)
        got = ctx.download(big_out)
        assert (got[:, :ow] == model(host[:h], ow, oh, F, S)).all() and (got[:, ow:] == SENTINEL).all()
    finally:
        for f in (mv, tall, big_in, big_out):
            ctx.destroy_frame(f)


# ---- 5. three lanes, tables and brackets rebuilt under frames in flight

def test_three_lanes_give_the_same(ctx):
    """More (in, out) pairs than the context keeps brackets for (14), with no sync between the calls: a bracket table is dropped
    and built while kernels that read others are queued on other lanes."""
    cases = [(13 + i, 7, 26 + 3 * i, 14 + i, RINGING[1 + i % 4], STRENGTHS[i % 3]) for i in range(18)]
    cases += [(67, 9, 130, 20, rm.LANCZOS3, 64), am.HORIZONTAL_ONLY + (rm.LANCZOS2, 24), am.VERTICAL_ONLY + (rm.MITCHELL, 64), cases[0]]
    inputs = [(rm.binary_noise(w, h, 900 + i),) for i, (w, h, *_) in enumerate(cases)]
    alone = []
    for (frame,), (w, h, ow, oh, filt, s) in zip(inputs, cases):
        alone.append(gpu(ctx, frame, ow, oh, filt, s))
        assert (alone[-1] == model(frame, ow, oh, filt, s)).all(), (w, h, ow, oh, rm.NAMES[filt], s)

    def enqueue(i, frame):
        _, _, ow, oh, filt, s = cases[i]
        f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
        ctx.resample_antiring(f, o, filt, s)
        return f, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- 6. 1080p -> 4K on regions of interest

def test_1080p_to_4k_on_eight_regions(ctx):
    w, h, ow, oh, n = 1920, 1080, 3840, 2160, 64
    frame = rm.binary_noise(w, h, 4)
    got = gpu(ctx, frame, ow, oh, rm.LANCZOS3, 64)
    rng = np.random.default_rng(12)
    regions = [(0, 0), (ow - n, 0), (0, oh - n), (ow - n, oh - n)] + [(int(rng.integers(0, ow - n)), int(rng.integers(0, oh - n))) for _ in range(4)]
    for x0, y0 in regions:
        want = model(frame, ow, oh, rm.LANCZOS3, 64, roi=(x0, y0, n, n))
        assert (got[y0:y0 + n, x0:x0 + n] == want).all(), f"region at {x0}, {y0}: {first_bad(got[y0:y0 + n, x0:x0 + n], want)}"
