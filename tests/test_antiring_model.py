"""lfg_resample_antiring where it needs no GPU: the library's one bracket builder (lfg_resample_brackets) against plain Python
integers, the lemma that lets the kernel read the bracket among the taps, and what the definition promises, shown on the model
(tests/antiring_model.py) -- whose bytes the GPU is held to.  CPU only."""
import functools
import os

import numpy as np
import pytest

from tests import antiring_model as am
from tests import resample_model as rm

RATIOS = rm.RATIOS + [(1, 1), (1, 7), (7, 8), (64, 65), (2, 6), (1080, 2160)]        # in = 1; out = in + 1; a centre on a texel
BOTH_GROW = [(5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (40, 9, 130, 20), (2, 2, 131, 67), (1, 1, 4, 3)]
ONE_GROWS = [am.HORIZONTAL_ONLY, am.VERTICAL_ONLY]
NONE_GROWS = [(24, 16, 24, 16), (37, 19, 12, 6)]
RINGING = tuple(f for f in rm.FILTERS if f != rm.NEAREST)
STRENGTHS = (1, 24, 32, 64)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as entry
    from linux_fg_amd import capi as c
    if not os.path.exists(c.LIB_PATH):
        entry.build()
    return c


@functools.lru_cache(maxsize=None)
def table(filt, n_in, n_out):
    return rm.table(filt, n_in, n_out)


def contents(w, h, seed):
    return (("binary noise", rm.binary_noise(w, h, seed)),
            ("random bytes", np.random.default_rng(seed + 1).integers(0, 256, (h, w, 4)).astype(np.uint8)))


def model(frame, ow, oh, filt, strength, bound=False):
    h, w = frame.shape[:2]
    return am.antiring(frame, ow, oh, filt, strength, table(filt, w, ow), table(filt, h, oh), bound)


def plain(frame, ow, oh, filt):
    h, w = frame.shape[:2]
    return rm.resample_int(frame, table(filt, w, ow), table(filt, h, oh))


def ids(shapes):
    return ["{}x{}-{}x{}".format(*s) for s in shapes]


# ---- 1. the brackets and the lemma

def test_the_librarys_brackets_are_the_models(capi):
    for n_in, n_out in RATIOS:
        lo, hi = capi.resample_brackets(n_in, n_out)
        a, b = am.brackets(n_in, n_out)
        assert lo.dtype == np.int32 and hi.dtype == np.int32 and (lo == a).all() and (hi == b).all(), (n_in, n_out)
        assert (0 <= a).all() and (a <= b).all() and (b <= n_in - 1).all() and (b - a <= 1).all(), (n_in, n_out)
    a, b = am.brackets(2, 6)                       # output 1 and 4 sit on the centres of texel 0 and 1: one texel, not two
    assert a.tolist() == [0, 0, 0, 0, 1, 1] and b.tolist() == [0, 0, 1, 1, 1, 1]
    assert a[1] == b[1] == 0 and a[4] == b[4] == 1


def test_the_bracket_builder_refuses(capi):
    import ctypes
    lib, buf = capi.load(), (ctypes.c_int32 * 4)()
    assert lib.lfg_resample_brackets(2, 4, None, buf) == capi.ERR_INVALID and lib.lfg_resample_brackets(2, 4, buf, None) == capi.ERR_INVALID
    assert lib.lfg_resample_brackets(0, 4, buf, buf) == capi.ERR_INVALID and lib.lfg_resample_brackets(2, 0, buf, buf) == capi.ERR_INVALID
    assert lib.lfg_resample_brackets(2 ** 31, 4, buf, buf) == capi.ERR_INVALID
    assert lib.lfg_resample_brackets(2 ** 31 - 1, 4, buf, buf) == 0 and list(buf) == am.brackets(2 ** 31 - 1, 4)[1].tolist()
    with pytest.raises(capi.LfgError):
        capi.resample_brackets(0, 4)


def test_the_bracket_lies_among_the_taps(capi):
    """first[p] <= a <= b < first[p] + count[p] on every growing axis, for every filter of support >= 1: on the model's tables
    and on the library's."""
    growing = [(i, o) for i, o in RATIOS if o > i]
    assert len(growing) >= 8
    for n_in, n_out in growing:
        a, b = am.brackets(n_in, n_out)
        for filt in RINGING:
            for first, count in (table(filt, n_in, n_out)[:2], capi.resample_taps(filt, n_in, n_out)[:2]):
                first, count = first.astype(np.int64), count.astype(np.int64)
                assert (first <= a).all() and (a <= b).all() and (b < first + count).all(), (rm.NAMES[filt], n_in, n_out)


# ---- 2. the literal step

def test_the_step_loses_its_halo():
    """24 x 12, 40 | 200, to 48 x 24 under Lanczos-3: 17 levels of halo on both sides without, half of them at S = 32, none at
    S = 64.  At 1.5 x and at 25 / 24 the halo is as deep within a level (the model gives 22 .. 218 at 1.5 x), and full strength
    removes it as exactly."""
    frame = am.step(24, 12, 40, 200)
    for ow, oh in ((48, 24), (36, 18), (25, 12)):
        got = {s: model(frame, ow, oh, rm.LANCZOS3, s) for s in (0, 32, 64)}
        assert (got[0] == plain(frame, ow, oh, rm.LANCZOS3)).all()
        ranges = {s: (int(g.min()), int(g.max())) for s, g in got.items()}
        print(f"step 24x12 -> {ow}x{oh}: {ranges}")
        if (ow, oh) == (48, 24):
            assert ranges == {0: (23, 217), 32: (32, 208), 64: (40, 200)}, ranges
        assert ranges[0][0] <= 24 and ranges[0][1] >= 216 and ranges[64] == (40, 200), (ow, oh, ranges)
        assert ranges[0][0] < ranges[32][0] < 40 and 200 < ranges[32][1] < ranges[0][1], (ow, oh, ranges)


# ---- 3. the consequences of the definition

@pytest.mark.parametrize("shape", BOTH_GROW, ids=ids(BOTH_GROW))
def test_full_strength_stays_within_the_four_texels(shape):
    w, h, ow, oh = shape
    (ax, bx), (ay, by) = am.brackets(w, ow), am.brackets(h, oh)
    for what, frame in contents(w, h, 10 * w + h):
        corners = np.stack([frame[ay][:, ax], frame[ay][:, bx], frame[by][:, ax], frame[by][:, bx]])
        for filt in RINGING:
            got = model(frame, ow, oh, filt, 64)
            assert (got >= corners.min(0)).all() and (got <= corners.max(0)).all(), (what, rm.NAMES[filt])


@pytest.mark.parametrize("shape", BOTH_GROW + ONE_GROWS, ids=ids(BOTH_GROW + ONE_GROWS))
def test_bilinear_and_nearest_are_untouched_and_unbound_bytes_are_plain(shape):
    w, h, ow, oh = shape
    for what, frame in contents(w, h, 20 * w + h):
        for filt in rm.FILTERS:
            want = plain(frame, ow, oh, filt)
            for s in STRENGTHS:
                got, bound = model(frame, ow, oh, filt, s, bound=True)
                if filt in (rm.NEAREST, rm.BILINEAR):
                    assert (got == want).all() and not bound.any(), (what, rm.NAMES[filt], s)
                assert (got[~bound] == want[~bound]).all(), (what, rm.NAMES[filt], s)


@pytest.mark.parametrize("shape", NONE_GROWS, ids=ids(NONE_GROWS))
def test_no_growing_axis_is_resample(shape):
    w, h, ow, oh = shape
    for what, frame in contents(w, h, 30 * w + h):
        for filt in rm.FILTERS:
            for s in (0,) + STRENGTHS:
                assert am.strengths(filt, w, h, ow, oh, s) == (0, 0)
                assert (model(frame, ow, oh, filt, s) == plain(frame, ow, oh, filt)).all(), (what, rm.NAMES[filt], s)


def test_strength_zero_is_resample_and_one_pass_alone_is_one_clamp():
    for shape in BOTH_GROW + ONE_GROWS:
        w, h, ow, oh = shape
        frame = rm.binary_noise(w, h, 40 * w + h)
        for filt in RINGING:
            assert (model(frame, ow, oh, filt, 0) == plain(frame, ow, oh, filt)).all()
    assert am.strengths(rm.LANCZOS3, *am.HORIZONTAL_ONLY, 64) == (64, 0) and am.strengths(rm.LANCZOS3, *am.VERTICAL_ONLY, 64) == (0, 64)
    # the vertical pass alone at full strength: every byte within the two h' of its bracket, that is within the plain horizontal
    # pass of the two source rows -- checked through a frame whose rows are constant, where that pass is the identity
    w, h, ow, oh = am.VERTICAL_ONLY
    frame = np.repeat(np.random.default_rng(5).integers(0, 256, (h, 1, 4)).astype(np.uint8), w, axis=1)
    a, b = am.brackets(h, oh)
    got = model(frame, ow, oh, rm.LANCZOS3, 64)
    assert (got >= np.minimum(frame[a, :1], frame[b, :1])).all() and (got <= np.maximum(frame[a, :1], frame[b, :1])).all()


def test_a_constant_frame_stays_constant():
    for w, h, ow, oh in BOTH_GROW + ONE_GROWS:
        for value in (0, 1, 127, 255):
            frame = np.full((h, w, 4), value, np.uint8)
            for filt in RINGING:
                for s in STRENGTHS:
                    assert (model(frame, ow, oh, filt, s) == value).all(), (w, h, ow, oh, rm.NAMES[filt], s, value)


def test_the_clamp_binds_where_it_should():
    """So that no comparison above passes because nothing happened: on binary noise under Lanczos-3 at full strength at least
    half of the pixels of 13 x 7 -> 26 x 14 differ from lfg_resample's, and a third where the vertical pass alone qualifies."""
    for shape, floor in (((13, 7, 26, 14), 1 / 2), (am.VERTICAL_ONLY, 1 / 3)):
        w, h, ow, oh = shape
        frame = rm.binary_noise(w, h, 50 * w + h)
        differ = (model(frame, ow, oh, rm.LANCZOS3, 64) != plain(frame, ow, oh, rm.LANCZOS3)).any(-1).mean()
        print(f"{w}x{h} -> {ow}x{oh}: {differ:.2f} of the pixels differ")
        assert differ >= floor, (shape, differ)


def test_a_region_of_interest_is_the_frames():
    frame = rm.binary_noise(40, 9, 3)
    whole = model(frame, 130, 20, rm.LANCZOS3, 24)
    for roi in ((0, 0, 64, 20), (66, 3, 64, 17), (100, 11, 30, 9)):
        x0, y0, rw, rh = roi
        part = am.antiring(frame, 130, 20, rm.LANCZOS3, 24, table(rm.LANCZOS3, 40, 130), table(rm.LANCZOS3, 9, 20), roi=roi)
        assert (part == whole[y0:y0 + rh, x0:x0 + rw]).all(), roi
