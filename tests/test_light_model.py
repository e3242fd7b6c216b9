"""lfg_resample_light where it needs no GPU: the library's one table builder (lfg_light_tables) against Python floats, and what the
definition gives and promises, shown on the model (tests/light_model.py) -- whose bytes the GPU is held to -- beside
lfg_resample's model, so that each test states the difference the feature makes.  CPU only."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import antiring_model as am
from tests import light_model as lm
from tests import resample_model as rm

FILTERS = tuple(f for f in rm.FILTERS if f != rm.NEAREST)
INTERPOLATING = (rm.BILINEAR, rm.CATMULL_ROM, rm.LANCZOS2, rm.LANCZOS3)
MORE_SHAPES = [(48, 27, 96, 54), (96, 54, 48, 27), (96, 54, 32, 18)]


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


@functools.lru_cache(maxsize=None)
def light_tables(mode):
    return lm.tables(mode)


def random_bytes(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def model(frame, ow, oh, filt, mode):
    h, w = frame.shape[:2]
    return lm.light(frame, ow, oh, filt, mode, table(filt, w, ow), table(filt, h, oh), None if mode == lm.GAMMA else light_tables(mode))


def plain(frame, ow, oh, filt):
    h, w = frame.shape[:2]
    return rm.resample_int(frame, table(filt, w, ow), table(filt, h, oh))


def modes(w, h, ow, oh):
    return lm.MODES if ow >= w and oh >= h else (lm.LINEAR,)


def unfolded(filt, n_in, n_out):
    """The output samples of an axis none of whose taps was folded onto the edge."""
    ranges = [rm.tap_range(filt, n_in, n_out, p) for p in range(n_out)]
    return [p for p, (k0, n) in enumerate(ranges) if k0 >= 0 and k0 + n <= n_in]


# ---- 1. the tables

def test_the_librarys_tables_are_the_models(capi):
    for mode in lm.MODES:
        forward, threshold = capi.light_tables(mode)
        f, t = lm.tables(mode)
        assert forward.dtype == np.uint16 and threshold.dtype == np.uint16 and forward.shape == (256,) and threshold.shape == (255,)
        assert (forward == f).all() and (threshold == t).all(), lm.NAMES[mode]


def test_the_table_builder_refuses(capi):
    lib, f, t = capi.load(), (ctypes.c_uint16 * 256)(), (ctypes.c_uint16 * 255)()
    for light in (capi.LIGHT_GAMMA, -1, 3):
        assert lib.lfg_light_tables(light, f, t) == capi.ERR_INVALID, light
    assert lib.lfg_light_tables(capi.LIGHT_LINEAR, None, t) == capi.ERR_INVALID and lib.lfg_light_tables(capi.LIGHT_LINEAR, f, None) == capi.ERR_INVALID
    assert lib.lfg_light_tables(capi.LIGHT_SIGMOID, f, t) == 0 and list(f) == lm.tables(lm.SIGMOID)[0].tolist()
    with pytest.raises(capi.LfgError):
        capi.light_tables(capi.LIGHT_GAMMA)
    assert (capi.LIGHT_GAMMA, capi.LIGHT_LINEAR, capi.LIGHT_SIGMOID) == (lm.GAMMA, lm.LINEAR, lm.SIGMOID)


def test_the_tables_entries_steps_and_round_trip():
    pinned = {lm.LINEAR: ([5, 10, 15], 3536, 8239, 5), lm.SIGMOID: ([83, 163, 241], 8571, 11514, 48)}
    for mode, (first, at128, at188, step) in pinned.items():
        forward, threshold = lm.tables(mode)
        assert forward[0] == 0 and forward[1:4].tolist() == first and forward[128] == at128 and forward[188] == at188 and forward[255] == lm.ONE
        assert np.diff(forward).min() == step and (np.diff(forward) > 0).all() and (np.diff(threshold) > 0).all()
        assert (lm.to_byte(forward, threshold) == np.arange(256)).all()
        every = lm.to_byte(np.arange(lm.ONE + 1), threshold)
        assert every[0] == 0 and every[-1] == 255 and (np.diff(every) >= 0).all()
        margin = lm.tie_margin(mode)
        print(f"{lm.NAMES[mode]}: nearest a value comes to a rounding tie {margin:.2e}")
        assert margin > 1e-4, margin                                  # far beyond a libm's error of a few 1e-12 at this magnitude


# ---- 2. the stripes and the step

def test_the_stripes_keep_their_light():
    """One-pixel stripes 0 | 255: half the light is the byte 188, where lfg_resample gives 128.  On the columns none of whose taps
    was folded onto the edge; at 3 : 1 bilinear weighs the stripes 4 : 5 and 5 : 4."""
    rows = {(24, 4, 12, 2, rm.BILINEAR): ({128}, {188}), (24, 4, 12, 2, rm.LANCZOS3): ({128}, {188}),
            (36, 6, 12, 2, rm.BILINEAR): ({113, 142}, {178, 197}), (36, 6, 12, 2, rm.LANCZOS3): ({127, 128}, {188})}
    for (w, h, ow, oh, filt), (want_plain, want_linear) in rows.items():
        frame = rm.stripes(w, h)
        inner = unfolded(filt, w, ow)
        assert len(inner) >= 4
        got_plain, got_linear = plain(frame, ow, oh, filt)[:, inner, :3], model(frame, ow, oh, filt, lm.LINEAR)[:, inner, :3]
        print(f"stripes {w}x{h} -> {ow}x{oh} {rm.NAMES[filt]}: lfg_resample {sorted(set(got_plain.ravel().tolist()))}, "
              f"linear {sorted(set(got_linear.ravel().tolist()))}")
        assert set(got_plain.ravel().tolist()) == want_plain and set(got_linear.ravel().tolist()) == want_linear, (w, ow, rm.NAMES[filt])
        with pytest.raises(ValueError):
            model(frame, ow, oh, filt, lm.SIGMOID)                    # refused: an axis shrinks


def test_the_step_in_the_three_domains():
    """40 | 200 upscaled 2 x under Lanczos-3: linear light's undershoot reaches black, the sigmoid compresses both ends."""
    frame = am.step(24, 12, 40, 200)
    ranges = {}
    for mode in (lm.GAMMA,) + lm.MODES:
        got = model(frame, 48, 24, rm.LANCZOS3, mode)[..., :3]
        ranges[lm.NAMES[mode]] = (int(got.min()), int(got.max()))
    print(f"step 24x12 -> 48x24: {ranges}")
    assert ranges == {"gamma": (23, 217), "linear": (0, 209), "sigmoid": (29, 216)}, ranges


# ---- 3. what follows from the definition

@pytest.mark.parametrize("shape", [(13, 7, 26, 14), (13, 7, 5, 3)], ids=["13x7-26x14", "13x7-5x3"])
def test_a_constant_frame_stays_constant(shape):
    w, h, ow, oh = shape
    for value in range(256):
        frame = np.full((h, w, 4), value, np.uint8)
        for mode in modes(*shape):
            for filt in FILTERS:
                assert (model(frame, ow, oh, filt, mode) == value).all(), (lm.NAMES[mode], rm.NAMES[filt], value)


def test_the_same_size_is_the_identity_under_an_interpolating_filter():
    for frame in (rm.binary_noise(24, 16, 1), random_bytes(24, 16, 2)):
        for mode in lm.MODES:
            for filt in INTERPOLATING:
                assert (model(frame, 24, 16, filt, mode) == frame).all(), (lm.NAMES[mode], rm.NAMES[filt])
            assert (model(frame, 24, 16, rm.MITCHELL, mode) != frame).any()                       # no interpolating kernel


def test_alpha_is_resamples_and_gamma_and_nearest_are_resample():
    for w, h, ow, oh in rm.SHAPES:
        frame = random_bytes(w, h, 300 * w + h)
        for filt in rm.FILTERS:
            want = plain(frame, ow, oh, filt)
            assert (model(frame, ow, oh, filt, lm.GAMMA) == want).all()
            for mode in modes(w, h, ow, oh):
                got = model(frame, ow, oh, filt, mode)
                assert (got[..., 3] == want[..., 3]).all(), (w, h, ow, oh, rm.NAMES[filt], lm.NAMES[mode])
                if filt == rm.NEAREST:
                    assert (got == want).all()


def test_binary_noise_differs_on_most_pixels():
    """So that no comparison passes because nothing happened: under Lanczos-3 the colour bytes differ from lfg_resample's on at
    least half the pixels."""
    for w, h, ow, oh in ((13, 7, 26, 14), (37, 19, 12, 6)):
        frame = rm.binary_noise(w, h, 50 * w + h)
        want = plain(frame, ow, oh, rm.LANCZOS3)
        for mode in modes(w, h, ow, oh):
            differ = (model(frame, ow, oh, rm.LANCZOS3, mode)[..., :3] != want[..., :3]).any(-1).mean()
            print(f"{w}x{h} -> {ow}x{oh} {lm.NAMES[mode]}: {differ:.2f} of the pixels differ")
            assert differ >= 0.5, (w, h, ow, oh, lm.NAMES[mode], differ)


def test_a_region_of_interest_is_the_frames():
    frame = rm.binary_noise(40, 9, 3)
    tx, ty = table(rm.LANCZOS3, 40, 130), table(rm.LANCZOS3, 9, 20)
    for mode in lm.MODES:
        whole = model(frame, 130, 20, rm.LANCZOS3, mode)
        for roi in ((0, 0, 64, 20), (66, 3, 64, 17), (100, 11, 30, 9)):
            x0, y0, rw, rh = roi
            assert (lm.light(frame, 130, 20, rm.LANCZOS3, mode, tx, ty, roi=roi) == whole[y0:y0 + rh, x0:x0 + rw]).all(), roi


# ---- 4. the distance to true linear-light filtering

def test_within_one_code_value_of_float64_linear_light():
    """The integer pipeline's colour bytes against float64 linear-light filtering with the unquantised weights, encoded and not
    rounded: below 1.0 of a code value, of which rounding to a byte alone is 0.5."""
    worst = (0.0, None)
    for w, h, ow, oh in rm.SHAPES + MORE_SHAPES:
        for what, frame in (("random bytes", random_bytes(w, h, 400 * w + h)), ("binary noise", rm.binary_noise(w, h, 500 * w + h))):
            for filt in FILTERS:
                tx, ty = table(filt, w, ow), table(filt, h, oh)
                got = lm.light(frame, ow, oh, filt, lm.LINEAR, tx, ty, light_tables(lm.LINEAR))[..., :3]
                d = float(np.abs(got.astype(np.float64) - lm.linear_f64(frame, tx, ty)).max())
                worst = max(worst, (d, (w, h, ow, oh, rm.NAMES[filt], what)))
    print(f"worst distance from float64 linear light: {worst[0]:.3f} of a code value at {worst[1]}")
    assert worst[0] < 1.0, worst
