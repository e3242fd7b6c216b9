"""The level-matching model (tests/levels_model.py) held to account before anything is held to it: the maps' properties, what
levelling does to a fade on the shared scenes (tests/levels_cases.py), the distance of every scene from the gate that the GPU
tests use it with, and the behaviour the feature is for -- the compensated chain finds its matches again.  CPU only."""
import numpy as np
import pytest

from tests import cases
from tests import levels_cases as lc
from tests import levels_model as lm
from tests import pair_model as pair

SIZES = [(64, 48), (200, 120)]
KINDS = ("textured", "noise")


def mean_shift16(m):
    return 16 * m["shift_sum"] / (3 * m["pixels"])


@pytest.mark.parametrize("name", list(lc.FADES))
@pytest.mark.parametrize("kind", KINDS)
def test_both_maps_are_monotone_and_compose_within_the_coarser_step(name, kind):
    """forward and inverse never decrease.  A fade of gain g / 256 puts at most ceil(256 / g) neighbouring levels of prev on one
    level of curr, whose running sum counts all of them, so inverse gives the largest of them back: inverse(forward(v)) is at
    most that many less one above v."""
    prev, curr = lc.faded_pan(64, 48, 5, name, kind)
    m = lm.pair_map(prev, curr, 0)
    assert m["active"] == 1 and m["reserved"] == 0 and m["pixels"] == 64 * 48
    for t in (m["forward"], m["inverse"]):
        assert (np.diff(t.astype(int), axis=1) >= 0).all()
    step = -(-256 // lc.FADES[name][0])
    occupied = lm.histogram(prev)[1][:3] > 0
    back = np.take_along_axis(m["inverse"], m["forward"].astype(np.int64), axis=1).astype(int)
    d = (back - np.arange(256)[None, :])[occupied]
    assert d.min() >= 0 and d.max() <= step - 1, (d.min(), d.max(), step)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_a_rolled_pan_has_equal_histograms_and_shift_zero(size, kind):
    prev, curr = lc.pan(*size, 3, kind)
    (pa, ha), (pb, hb) = lm.histogram(prev), lm.histogram(curr)
    assert pa == pb == size[0] * size[1] and (ha == hb).all()
    m = lm.match((pa, ha), (pb, hb), 0)
    assert m["shift_sum"] == 0 and m["active"] == 1
    occupied = ha[:3] > 0                                # an identity on every level that a pixel has
    assert (m["forward"][occupied] == np.broadcast_to(np.arange(256), (3, 256))[occupied]).all()
    assert (lm.apply(prev, m, lm.FORWARD) == prev).all()
    assert lm.match((pa, ha), (pb, hb), 1)["active"] == 0


@pytest.mark.parametrize("name", list(lc.FADES))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
def test_forward_brings_a_faded_pan_within_one_level_of_curr(name, size, kind):
    prev, curr = lc.faded_pan(*size, 5, name, kind)
    m = lm.pair_map(prev, curr, lc.THRESHOLD)
    assert m["active"] == 1
    levelled = lc.rolled(lm.apply(prev, m, lm.FORWARD), *lc.PAN)
    assert (levelled[..., 3] == curr[..., 3]).all()
    off_clip = (curr[..., :3] > 0) & (curr[..., :3] < 255)
    d = np.abs(levelled[..., :3].astype(int) - curr[..., :3].astype(int))
    print(f"{name} {size} {kind}: max {d[off_clip].max()}, mean {d.mean():.3f}, mean shift {mean_shift16(m) / 16:.2f} levels")
    assert d[off_clip].max() <= 1


@pytest.mark.parametrize("name", list(lc.FADES))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_at_half_takes_a_compensated_frame_within_one_level_of_the_true_halfway_frame(name, size):
    prev, curr, compensated, true = lc.halfway(*size, 5, name)
    m = lm.pair_map(prev, curr, lc.THRESHOLD)
    got = lm.apply(compensated, m, lm.AT, 0.5)
    d = np.abs(got[..., :3].astype(int) - true[..., :3].astype(int))
    without = np.abs(compensated[..., :3].astype(int) - true[..., :3].astype(int))
    print(f"{name} {size}: with the map max {d.max()} mean {d.mean():.3f}; without it mean {without.mean():.2f}")
    assert d.max() <= 1 and d.mean() < without.mean() / 4
    assert (got[..., 3] == compensated[..., 3]).all()
    assert (lm.apply(compensated, m, lm.AT, 1.0) == compensated).all()          # t = 1 leaves a frame as it is


def test_tq_rounds_to_nearest_in_fp32():
    assert [lm.tq_of(f) for f in lc.FACTORS] == [0, 1, 64, 128, 256, 256]
    assert lm.tq_of(0.5 / 256) == 1 and lm.tq_of(0.25 / 256) == 0 and lm.tq_of(0.75 / 256) == 1
    # the sum is an fp32 sum: for the float just below half a step, factor * 256 + 0.5 rounds to 1.0f, and so tq = 1 as well
    assert lm.tq_of(float(np.nextafter(np.float32(0.5 / 256), np.float32(0)))) == 1


@pytest.mark.parametrize("name", list(lc.record_pairs()))
def test_hand_made_records(name):
    a, b = lc.record_pairs()[name]
    for s in lc.MIN_SHIFTS:
        m = lm.match(a, b, s)
        identity = (m["forward"] == np.arange(256, dtype=np.uint8)).all() and (m["inverse"] == np.arange(256, dtype=np.uint8)).all()
        assert m["pixels"] == a[0] and (m["active"] == 1 or identity)
        if name in ("pixels_differ", "pixels_zero", "from_empty"):
            assert m["active"] == 0
    if name == "single_levels":                          # A all 10, B all 200: 190 levels on every pixel of three channels
        m = lm.match(a, b, 190 * 16)
        assert m["active"] == 1 and m["shift_sum"] == 190 * 3 * 4096 and (m["forward"][:, 10] == 200).all() and (m["inverse"][:, 200] == 10).all()
        assert lm.match(a, b, 190 * 16 + 1)["active"] == 0


def test_every_scene_lies_a_factor_two_from_the_gate_it_is_used_with():
    """No GPU test sits on the gate's edge: 16 * shift_sum against min_shift16 * 3 * pixels, a factor 2 on the intended side."""
    for name, (prev, curr, threshold) in lc.switch_scenes().items():
        m = lm.pair_map(prev, curr, threshold)
        lhs, rhs = 16 * m["shift_sum"], threshold * 3 * m["pixels"]
        if name == "faded":
            assert m["active"] == 1 and lhs >= 2 * rhs, (name, lhs, rhs)
        elif threshold > 0:
            assert m["active"] == 0 and 2 * lhs <= rhs, (name, lhs, rhs)
        else:
            assert m["active"] == 1 and m["shift_sum"] == 0, name          # threshold 0: active, and an identity on the content
    frames = lc.fade_stream()
    for k in range(1, len(frames)):
        m = lm.pair_map(frames[k - 1], frames[k], lc.THRESHOLD)
        lhs, rhs = 16 * m["shift_sum"], lc.THRESHOLD * 3 * m["pixels"]
        assert lhs >= 2 * rhs if m["active"] else 2 * lhs <= rhs, (k, lhs, rhs)
    for name in lc.FADES:
        for size in SIZES:
            m = lm.pair_map(*lc.faded_pan(*size, 5, name), lc.THRESHOLD)
            assert 16 * m["shift_sum"] >= 2 * lc.THRESHOLD * 3 * m["pixels"], (name, size)


def test_the_wrapper_gives_the_plain_call_on_an_inactive_pair_and_curr_at_one():
    prev, curr = lc.pan(64, 48, 3)
    blend = lambda p, c: [((p.astype(int) + c.astype(int)) // 2).astype(np.uint8), c]
    outs, m = lm.wrapper(prev, curr, lc.THRESHOLD, blend, [0.5, 1.0])
    assert m["active"] == 0 and all((o == w).all() for o, w in zip(outs, blend(prev, curr)))
    prev, curr = lc.faded_pan(64, 48, 3)
    outs, m = lm.wrapper(prev, curr, lc.THRESHOLD, blend, [0.5, 1.0])
    assert m["active"] == 1 and (outs[1] == curr).all() and not (outs[0] == blend(prev, curr)[0]).all()
    shown, _ = lm.wrapper(prev, curr, lc.THRESHOLD, blend, [0.25, 0.5], cut=lambda p, c: True)
    assert shown[0] is prev and shown[1] is curr                           # a cut shows the caller's frames


def test_levelling_gives_the_compensated_chain_its_matches_back():
    """The behavioural test.  On the 200 x 120 faded pan the compensated chain (pyramid, intended semantics, match_sad 48) passes
    the match gate at fewer than 300 of a thousand pixels as it is and at more than 750 with the wrapper, and its frame at 0.5
    is nearer the true half-way frame with the wrapper than without."""
    w, h = lc.SCENE
    setting = ("pyramid", -1, "compensated", 1)
    prev, curr, _, true = lc.halfway(w, h, 11)
    seen = {}

    def permille(p, c):
        chain = cases.Chain(p, c)
        return pair.permille(pair.pair_stats(p, c, chain.vectors("pyramid", -1, 1), 48)), chain

    def call(p, c):
        seen["permille"], chain = permille(p, c)
        return chain.frames(setting, [0.5])

    plain_permille, plain_chain = permille(prev, curr)
    plain = plain_chain.frames(setting, [0.5])[0]
    levelled, m = lm.wrapper(prev, curr, lc.THRESHOLD, call, [0.5])
    print(f"matched per thousand: {plain_permille} as it is, {seen['permille']} levelled; mean shift {mean_shift16(m) / 16:.1f} levels")
    assert m["active"] == 1 and plain_permille < 300 and seen["permille"] > 750

    def sse(f):
        return int(((f[..., :3].astype(np.int64) - true[..., :3].astype(np.int64)) ** 2).sum())

    print(f"squared error against the true half-way frame: {sse(plain)} as it is, {sse(levelled[0])} levelled")
    assert sse(levelled[0]) < sse(plain)
