"""lfg_resample_light on the GPU, byte for byte against the CPU model (tests/light_model.py) run on the library's own taps and
tables: the smallest shapes at which each path can break, both modes and the five filters with sums to form; where the call is
lfg_resample; what the definition promises, on the GPU's own output; padded pitches and views; argument checks; three lanes;
and one 1080p -> 4K and one 4K -> 1080p call on eight regions of interest each."""
import ctypes
import functools

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import light_model as lm
from tests import resample_model as rm
from tests.gpu_kit import ctx, first_bad, pitched, three_lanes

pytestmark = pytest.mark.gpu

SENTINEL = rm.SENTINEL
GROWING = [(1, 1, 4, 3), (5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (24, 16, 24, 16), (33, 5, 65, 9), (70, 6, 64, 4), (67, 9, 130, 20),
           (2, 2, 131, 67)]
SHRINKING = [(37, 19, 12, 6), (64, 9, 8, 3), (96, 8, 9, 2)] + [rm.SMALL_T[rows] for rows in (4, 2, 1)]
FILTERS = tuple(f for f in rm.FILTERS if f != rm.NEAREST)
INTERPOLATING = (rm.BILINEAR, rm.CATMULL_ROM, rm.LANCZOS2, rm.LANCZOS3)


@functools.lru_cache(maxsize=None)
def taps(filt, n_in, n_out):
    return capi.resample_taps(filt, n_in, n_out)


@functools.lru_cache(maxsize=None)
def light_tables(mode):
    return capi.light_tables(mode)


def modes(w, h, ow, oh):
    """Both where no axis shrinks.  (70, 6, 64, 4) stands among the growing shapes for its tile-wide output, but both of its axes
    shrink: the sigmoid is refused there (test_invalid_arguments_launch_nothing) and linear light alone runs."""
    return lm.MODES if ow >= w and oh >= h else (lm.LINEAR,)


def model(frame, ow, oh, filt, mode, roi=None):
    h, w = frame.shape[:2]
    return lm.light(frame, ow, oh, filt, mode, taps(filt, w, ow), taps(filt, h, oh), None if mode == lm.GAMMA else light_tables(mode), roi=roi)


def random_bytes(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def gpu(ctx, frame, ow, oh, filt, mode=None):
    """lfg_resample_light of `frame`, or lfg_resample with mode=None, through tight frames."""
    f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
    try:
        if mode is None:
            ctx.resample(f, o, filt)
        else:
            ctx.resample_light(f, o, filt, mode)
        return ctx.download(o)
    finally:
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


def ids(shapes):
    return ["{}x{}-{}x{}".format(*s) for s in shapes]


# ---- 1. bytes equal the model

def test_the_constants_and_the_tables_are_the_models():
    assert (capi.LIGHT_GAMMA, capi.LIGHT_LINEAR, capi.LIGHT_SIGMOID) == (lm.GAMMA, lm.LINEAR, lm.SIGMOID)
    for mode in lm.MODES:
        assert all((a == b).all() for a, b in zip(light_tables(mode), lm.tables(mode)))


@pytest.mark.parametrize("shape", GROWING + SHRINKING, ids=ids(GROWING + SHRINKING))
def test_equals_the_model(ctx, shape):
    w, h, ow, oh = shape
    noise, rand = rm.binary_noise(w, h, 100 * w + h), random_bytes(w, h, 200 * w + h)
    f, g, o = ctx.frame_from(noise), ctx.frame_from(rand), ctx.create_frame(ow, oh)
    try:
        for mode in modes(*shape):
            for filt in FILTERS:
                for frame, src in ((noise, f), (rand, g)):
                    ctx.resample_light(src, o, filt, mode)
                    got, want = ctx.download(o), model(frame, ow, oh, filt, mode)
                    assert (got == want).all(), f"{w}x{h}->{ow}x{oh} {rm.NAMES[filt]} {lm.NAMES[mode]}: {first_bad(got, want)}"
    finally:
        for frame in (f, g, o):
            ctx.destroy_frame(frame)


@pytest.mark.parametrize("case", [(960, 540, lm.SIGMOID), (160, 90, lm.LINEAR)], ids=["up-sigmoid", "down-linear"])
def test_a_quarter_of_1080p_equals_the_model(ctx, case):
    ow, oh, mode = case
    frame = random_bytes(480, 270, 9)
    got, want = gpu(ctx, frame, ow, oh, rm.LANCZOS3, mode), model(frame, ow, oh, rm.LANCZOS3, mode)
    assert (got == want).all(), first_bad(got, want)


# ---- 2. where it is lfg_resample, and what the definition promises

def test_gamma_and_nearest_are_resample(ctx):
    for w, h, ow, oh in [(13, 7, 26, 14), (13, 7, 17, 10), (24, 16, 24, 16), (37, 19, 12, 6)]:
        frame = random_bytes(w, h, 3 * w + h)
        for filt in rm.FILTERS:
            want = gpu(ctx, frame, ow, oh, filt)
            assert (gpu(ctx, frame, ow, oh, filt, lm.GAMMA) == want).all(), (w, h, ow, oh, rm.NAMES[filt])
        for mode in lm.MODES:                                         # NEAREST shrinks under the sigmoid too: it is lfg_resample
            assert (gpu(ctx, frame, ow, oh, rm.NEAREST, mode) == gpu(ctx, frame, ow, oh, rm.NEAREST)).all(), (w, h, ow, oh, lm.NAMES[mode])
    frame = rm.binary_noise(13, 7, 72)                                # and where it is not: most pixels differ
    for mode in lm.MODES:
        differ = (gpu(ctx, frame, 26, 14, rm.LANCZOS3, mode)[..., :3] != gpu(ctx, frame, 26, 14, rm.LANCZOS3)[..., :3]).any(-1).mean()
        assert differ >= 0.5, (lm.NAMES[mode], differ)


def test_timed_as_the_scale_stage_in_one_launch(ctx):
    f, o = ctx.frame_from(rm.binary_noise(13, 7, 1)), ctx.create_frame(17, 10)
    try:
        launches = ctypes.c_uint64()
        for mode in (lm.GAMMA,) + lm.MODES:
            assert ctx.lib.lfg_profile_enable(ctx.h, 1) == 0 and ctx.lib.lfg_profile_reset(ctx.h) == 0
            ctx.resample_light(f, o, capi.FILTER_LANCZOS3, mode)
            assert ctx.lib.lfg_profile_get(ctx.h, capi.STAGE_SCALE, None, ctypes.byref(launches)) == 0 and launches.value == 1, lm.NAMES[mode]
    finally:
        ctx.lib.lfg_profile_enable(ctx.h, 0)
        ctx.destroy_frame(f)
        ctx.destroy_frame(o)


def test_constants_identity_alpha_and_the_stripes(ctx):
    for w, h, ow, oh in ((13, 7, 26, 14), (13, 7, 5, 3)):
        for value in (0, 1, 2, 127, 128, 254, 255):
            for mode in modes(w, h, ow, oh):
                for filt in (rm.BILINEAR, rm.MITCHELL, rm.LANCZOS3):
                    assert (gpu(ctx, np.full((h, w, 4), value, np.uint8), ow, oh, filt, mode) == value).all(), (value, lm.NAMES[mode], rm.NAMES[filt])
    frame = random_bytes(24, 16, 5)
    for mode in lm.MODES:
        for filt in INTERPOLATING:
            assert (gpu(ctx, frame, 24, 16, filt, mode) == frame).all(), (lm.NAMES[mode], rm.NAMES[filt])
    for w, h, ow, oh in ((13, 7, 17, 10), (67, 9, 130, 20), (37, 19, 12, 6)):
        frame = random_bytes(w, h, 7 * w + h)
        for mode in modes(w, h, ow, oh):
            for filt in FILTERS:
                assert (gpu(ctx, frame, ow, oh, filt, mode)[..., 3] == gpu(ctx, frame, ow, oh, filt)[..., 3]).all(), (w, h, lm.NAMES[mode], rm.NAMES[filt])
    stripes = rm.stripes(24, 4)                                       # half the light: 188, not 128
    for filt, inner in ((rm.BILINEAR, slice(1, -1)), (rm.LANCZOS3, slice(3, -3))):
        assert (gpu(ctx, stripes, 12, 2, filt)[:, inner, :3] == 128).all() and (gpu(ctx, stripes, 12, 2, filt, lm.LINEAR)[:, inner, :3] == 188).all()


# ---- 3. padded pitches and views

def test_padded_pitches_keep_their_padding(ctx):
    for (w, h, ow, oh), pad_in, pad_out, mode in (((33, 5, 65, 9), 3, 5, lm.SIGMOID), ((13, 7, 26, 14), 1, 7, lm.LINEAR), ((37, 19, 12, 6), 2, 1, lm.LINEAR)):
        frame = random_bytes(w, h, 11 * w + h)
        big_in, src = pitched(ctx, frame, pad_in)
        big_out, dst = pitched(ctx, np.full((oh, ow, 4), SENTINEL, np.uint8), pad_out)
        try:
            ctx.resample_light(src, dst, capi.FILTER_LANCZOS3, mode)
            got, kept = ctx.download(big_out), ctx.download(big_in)
            want = model(frame, ow, oh, rm.LANCZOS3, mode)
            assert (got[:, :ow] == want).all(), first_bad(got[:, :ow], want)
            assert (got[:, ow:] == SENTINEL).all(), "the output's padding was written"
            assert (kept[:, :w] == frame).all() and (kept[:, w:] == SENTINEL).all()
        finally:
            ctx.destroy_frame(big_in)
            ctx.destroy_frame(big_out)


def test_a_view_is_its_own_image(ctx):
    big_w, big_h, w, h, x0, y0, ow, oh = 40, 12, 13, 7, 3, 2, 29, 15
    inside = random_bytes(w, h, 77)
    results = []
    for outside in (0xFF, 0x00):
        big = np.full((big_h, big_w, 4), outside, np.uint8)
        big[y0:y0 + h, x0:x0 + w] = inside
        src, dst = ctx.frame_from(big), ctx.frame_from(np.full((big_h + oh, big_w, 4), SENTINEL, np.uint8))
        try:
            view_in = capi.Context.wrap(src.data + (y0 * big_w + x0) * 4, w, h, pitch=big_w * 4)
            view_out = capi.Context.wrap(dst.data + (y0 * big_w + x0) * 4, ow, oh, pitch=big_w * 4)
            ctx.resample_light(view_in, view_out, capi.FILTER_LANCZOS3, lm.SIGMOID)
            got = ctx.download(dst)
            results.append(got[y0:y0 + oh, x0:x0 + ow].copy())
            got[y0:y0 + oh, x0:x0 + ow] = SENTINEL
            assert (got == SENTINEL).all() and (ctx.download(src) == big).all()
        finally:
            ctx.destroy_frame(src)
            ctx.destroy_frame(dst)
    assert (results[0] == results[1]).all() and (results[0] == model(inside, ow, oh, rm.LANCZOS3, lm.SIGMOID)).all()


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
    narrow_out = capi.Context.wrap(big_out.data, w - 1, oh, pitch=good_out.pitch)       # the width shrinks, the height grows
    small_out = capi.Context.wrap(big_out.data, w - 1, h - 1, pitch=good_out.pitch)     # both shrink
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    F, L = capi.FILTER_CATMULL_ROM, capi.LIGHT_LINEAR
    try:
        def framed(like, ptr=None, width=None, height=None, pitch=None):
            f = capi.Frame()
            f.data, f.width, f.height = like.data if ptr is None else ptr, like.width if width is None else width, like.height if height is None else height
            f.pitch, f.format = pitch or like.pitch, capi.FORMAT_RGBA8
            return f

        no_data = framed(good_in)
        no_data.data = None
        calls = [(ctx.h, B(good_in), B(good_out), F, -1), (ctx.h, B(good_in), B(good_out), F, 3), (ctx.h, B(good_in), B(good_out), F, 1000),   # unknown lights
                 (ctx.h, B(good_in), B(good_out), capi.FILTER_NEAREST, 3),                                     # ... also where the light would not matter
                 (None, B(good_in), B(good_out), F, L), (ctx.h, None, B(good_out), F, L), (ctx.h, B(good_in), None, F, L),
                 (ctx.h, B(no_data), B(good_out), F, L), (ctx.h, B(good_in), B(no_data), F, L),
                 (ctx.h, B(mv), B(good_out), F, L), (ctx.h, B(good_in), B(mv), F, L),                          # MV_S8X2 on either side
                 (ctx.h, B(framed(good_in, width=0)), B(good_out), F, L), (ctx.h, B(good_in), B(framed(good_out, height=0)), F, L),
                 (ctx.h, B(framed(good_in, ptr=good_in.data + 2)), B(good_out), F, L), (ctx.h, B(good_in), B(framed(good_out, ptr=good_out.data + 2)), F, L),
                 (ctx.h, B(framed(good_in, pitch=good_in.pitch + 2)), B(good_out), F, L), (ctx.h, B(good_in), B(framed(good_out, pitch=good_out.pitch + 2)), F, L),
                 (ctx.h, B(framed(good_in, pitch=w * 4 - 4)), B(good_out), F, L), (ctx.h, B(good_in), B(framed(good_out, pitch=ow * 4 - 4)), F, L),
                 (ctx.h, B(good_in), B(good_in), F, L),                                                        # in place
                 (ctx.h, B(good_in), B(framed(good_in, ptr=good_in.data + good_in.pitch)), F, L),              # out one row into in
                 (ctx.h, B(good_in), B(good_out), -1, L), (ctx.h, B(good_in), B(good_out), 6, L)]              # unknown filters
        results = [lib.lfg_resample_light(*c) for c in calls]
        assert all(rc == capi.ERR_INVALID for rc in results), results
        assert "lfg_resample_light" in lib.lfg_last_error(ctx.h).decode()
        for out in (narrow_out, small_out):                           # the sigmoid where one axis shrinks, and where both do
            assert lib.lfg_resample_light(ctx.h, B(good_in), B(out), F, capi.LIGHT_SIGMOID) == capi.ERR_UNSUPPORTED
            assert "lfg_resample_light" in lib.lfg_last_error(ctx.h).decode()
        assert lib.lfg_resample_light(ctx.h, B(tall), B(short_out), capi.FILTER_LANCZOS3, L) == capi.ERR_UNSUPPORTED   # a refused table
        assert lib.lfg_last_error(ctx.h).decode()
        ctx.sync()
        assert (ctx.download(big_out) == SENTINEL).all() and (ctx.download(big_in)[:, :w] == host).all()
        ctx.resample(good_in, good_out, F)                            # a valid call next to the bad ones works, plain and in both lights
        want = rm.resample_int(host[:h], taps(F, w, ow), taps(F, h, oh))
        assert (ctx.download(big_out)[:, :ow] == want).all()
        for mode in lm.MODES:
            ctx.resample_light(good_in, good_out, F, mode)
            got = ctx.download(big_out)
            assert (got[:, :ow] == model(host[:h], ow, oh, F, mode)).all() and (got[:, ow:] == SENTINEL).all()
    finally:
        for f in (mv, tall, big_in, big_out):
            ctx.destroy_frame(f)


# ---- 5. three lanes, tables rebuilt under frames in flight

def test_three_lanes_give_the_same(ctx):
    """More (filter, in, out) triples than the context keeps tables for (14), both modes mixed and no sync between the calls: a
    table is dropped and built while kernels that read others are queued on other lanes."""
    cases = [(13 + i, 7, 26 + 3 * i, 14 + i, FILTERS[1 + i % 4], lm.MODES[i % 2]) for i in range(18)]
    cases += [(67, 9, 130, 20, rm.LANCZOS3, lm.SIGMOID), (37, 19, 12, 6, rm.LANCZOS2, lm.LINEAR), (26, 13, 13, 26, rm.MITCHELL, lm.LINEAR), cases[0]]
    inputs = [(random_bytes(w, h, 900 + i),) for i, (w, h, *_) in enumerate(cases)]
    alone = []
    for (frame,), (w, h, ow, oh, filt, mode) in zip(inputs, cases):
        alone.append(gpu(ctx, frame, ow, oh, filt, mode))
        assert (alone[-1] == model(frame, ow, oh, filt, mode)).all(), (w, h, ow, oh, rm.NAMES[filt], lm.NAMES[mode])

    def enqueue(i, frame):
        _, _, ow, oh, filt, mode = cases[i]
        f, o = ctx.frame_from(frame), ctx.create_frame(ow, oh)
        ctx.resample_light(f, o, filt, mode)
        return f, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- 6. 1080p <-> 4K on regions of interest

@pytest.mark.parametrize("case", [(1920, 1080, 3840, 2160, lm.SIGMOID), (3840, 2160, 1920, 1080, lm.LINEAR)], ids=["1080p-4k-sigmoid", "4k-1080p-linear"])
def test_large_shapes_on_eight_regions(ctx, case):
    w, h, ow, oh, mode = case
    n = 64
    frame = random_bytes(w, h, 4)
    got = gpu(ctx, frame, ow, oh, rm.LANCZOS3, mode)
    rng = np.random.default_rng(12)
    regions = [(0, 0), (ow - n, 0), (0, oh - n), (ow - n, oh - n)] + [(int(rng.integers(0, ow - n)), int(rng.integers(0, oh - n))) for _ in range(4)]
    for x0, y0 in regions:
        want = model(frame, ow, oh, rm.LANCZOS3, mode, roi=(x0, y0, n, n))
        assert (got[y0:y0 + n, x0:x0 + n] == want).all(), f"region at {x0}, {y0}: {first_bad(got[y0:y0 + n, x0:x0 + n], want)}"
