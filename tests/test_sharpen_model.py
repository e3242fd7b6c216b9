"""tests/sharpen_model.py against known answers, and the power of the inputs it shares with the GPU tests: each of them must
tell the definition from its mutants.  CPU only."""
import numpy as np
import pytest

from tests import sharpen_model as sm


def grey(rows):
    """A frame whose four channels all hold `rows` (a 2-D list or array of bytes)."""
    return np.repeat(np.asarray(rows, np.uint8)[:, :, None], 4, axis=2)


def test_strength_0_is_the_identity():
    for frame in (sm.noise(9, 5, 1), sm.smooth_scene(13, 7, 2)):
        assert (sm.sharpen(frame, 0) == frame).all()


def test_a_constant_frame_is_unchanged():
    frame = np.full((5, 6, 4), 77, np.uint8)
    assert (sm.sharpen(frame, 64) == frame).all()


def test_a_ramp_is_unchanged_everywhere():
    frame = grey([[10 + 7 * x for x in range(12)]] * 4)       # the clamped edges: L = -+7, limited to the end's own value
    assert (sm.sharpen(frame, 64) == frame).all()
    assert (sm.sharpen(frame.transpose(1, 0, 2).copy(), 64) == frame.transpose(1, 0, 2)).all()


def test_a_hard_step_is_unchanged():
    frame = grey([[100] * 4 + [200] * 4] * 3)
    for strength in (1, 32, 64):
        assert (sm.sharpen(frame, strength) == frame).all()


@pytest.mark.parametrize("strength", [32, 64])
def test_a_soft_edge_steepens_to_the_limit(strength):
    frame = grey([[100, 100, 110, 150, 190, 200, 200]] * 3)
    assert sm.sharpen(frame, strength)[1, :, 0].tolist() == [100, 100, 100, 150, 200, 200, 200]


def test_impulses_are_unchanged():
    for frame in sm.impulses():
        assert (sm.sharpen(frame, 64) == frame).all()


def test_every_byte_stays_in_the_range_of_its_neighbourhood():
    for seed, (w, h) in enumerate([(1, 1), (2, 5), (17, 9), (40, 23)]):
        frame = sm.noise(w, h, 50 + seed)
        p = np.pad(frame, ((1, 1), (1, 1), (0, 0)), mode="edge")
        five = np.stack([frame, p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]])
        for strength in range(sm.MAX_STRENGTH + 1):
            out = sm.sharpen(frame, strength)
            assert (out >= five.min(0)).all() and (out <= five.max(0)).all()
            assert (out.min((0, 1)) == frame.min((0, 1))).all() and (out.max((0, 1)) == frame.max((0, 1))).all()


def test_an_upscaled_edge(oracle):
    """The anti-aliased step 60 | 130 | 200 of 24 x 12, upscaled to 48 x 24: ... 55 70 108 152 190 205 ... through the edge."""
    small = grey([[60] * 11 + [130] + [200] * 12] * 12)
    up = oracle.scale(small, 48, 24)
    out = sm.sharpen(up, 32)
    before, after = up[12, :, 0].astype(int).tolist(), out[12, :, 0].astype(int).tolist()
    print("row 12 before", before, "after", after)
    for frame in (up, out):
        assert frame[..., :3].min() == 55 and frame[..., :3].max() == 205
    k = before.index(108)
    assert before[k - 2:k + 4] == [55, 70, 108, 152, 190, 205]
    assert after[k - 2:k + 4] == [55, 59, 105, 155, 202, 205]
    assert after[k + 1] - after[k] == 50 and before[k + 1] - before[k] == 44
    for strength in range(sm.MAX_STRENGTH + 1):
        s = sm.sharpen(up, strength)
        assert s.min() == up.min() and s.max() == up.max()


SCENES = [(13, 7, 1307), (67, 9, 6709)]


@pytest.mark.parametrize("mutant", ["zero_border", "truncating_shift", "byte_clamp"])
def test_the_shared_scenes_tell_the_mutants_apart(mutant):
    """Found with this generator (bytes that differ from the definition, of 364 and 2,412):
                         13 x 7 at 16, 37     67 x 9 at 16, 37
      zero_border             119, 97              493, 439
      truncating_shift        103, 105             725, 787
      byte_clamp              53, 140              304, 760"""
    for w, h, seed in SCENES:
        frame = sm.smooth_scene(w, h, seed)
        for strength in (16, 37):
            differing = int((sm.sharpen(frame, strength) != sm.sharpen(frame, strength, mutant)).sum())
            print(mutant, w, h, strength, differing)
            assert differing >= 10, (mutant, w, h, strength)


def test_the_scenes_change_under_the_sharpener_and_seldom_reach_the_limit():
    for w, h, seed in SCENES:
        frame = sm.smooth_scene(w, h, seed)
        assert (sm.sharpen(frame, 16) != frame).mean() > 0.5


def test_the_impulses_tell_a_16_bit_product_apart():
    """64 * 1020 = 65,280 wraps to -256 in 16 bits: the centre of the impulse would move by -4 (and +4)."""
    for frame in sm.impulses():
        assert (sm.sharpen(frame, 64) != sm.sharpen(frame, 64, "int16_product")).any()
