"""The CPU model of lfg_pair_match / lfg_cut_fallback (tests/pair_model.py): its gate is the compensated model's gate, hand
cases with literal values, the separation between moving content and cuts that the GPU tests' threshold of 500 rests on, and
the decision's boundary in exact integers.  CPU only."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import cases
from tests import mc_model as mc
from tests import pair_model as pair
from tests import pyramid_model as pm

MATCH_SADS = [0, 48, 1020]


# ---- the model's gate is the compensated model's gate: at t = 1 a matched pixel projects onto itself (s = 0), so the key
# image of tests/mc_model.c has a hole exactly where the pixel is unmatched

@pytest.mark.parametrize("name", ["random", "piecewise", "sampling"])
def test_gate_is_the_compensated_models_gate(name):
    if name == "sampling":
        prev, curr, mv = cases.sampling_scene_of(64, 36)
    else:
        prev, curr, mv = cases.field(name, 257, 131, 3 if name == "random" else 4)
    for sad in MATCH_SADS:
        want = mc.keys(prev, curr, mv, 1.0, sad) != mc.HOLE
        got = pair.matched_mask(prev, curr, mv, sad)
        assert (got == want).all(), (name, sad, int((got != want).sum()))
        assert pair.pair_stats(prev, curr, mv, sad)[1] == int(want.sum())
    assert pair.pair_stats(prev, curr, mv, 1020)[1] == prev.shape[0] * prev.shape[1]      # 4 * 255: nothing can exceed it


# ---- hand cases, literal values

def frame(h, w, value):
    f = np.zeros((h, w, 4), np.uint8)
    f[...] = value
    return f


def test_vector_that_leaves_the_image_reads_zero():
    prev = frame(4, 6, (200, 200, 200, 200))
    mv = np.zeros((4, 6, 2), np.int8)
    mv[1, 2] = (10, 0)                                    # (2, 1) + (10, 0) is outside: prev reads (0, 0, 0, 0) there
    curr = prev.copy()
    curr[1, 2] = (0, 0, 0, 0)
    assert pair.sad_map(prev, curr, mv)[1, 2] == 0
    assert pair.pair_stats(prev, curr, mv, 0) == (24, 24, 0)
    curr[1, 2] = (1, 0, 0, 0)
    assert pair.sad_map(prev, curr, mv)[1, 2] == 1
    assert pair.pair_stats(prev, curr, mv, 1) == (24, 24, 1)
    assert pair.pair_stats(prev, curr, mv, 0) == (24, 23, 1)
    mv[1, 2] = (0, 0)                                     # the same pixel against prev itself: 199 + 3 * 200
    assert pair.pair_stats(prev, curr, mv, 798) == (24, 23, 799)
    assert pair.pair_stats(prev, curr, mv, 799) == (24, 24, 799)


def test_byte_vectors_of_minus_128_and_127():
    w, h = 300, 3
    prev = cases.textured(w, h, 70)
    curr = np.zeros_like(prev)
    mv = np.zeros((h, w, 2), np.int8)
    mv[1, 200] = (-128, 0)
    curr[1, 200] = prev[1, 72]
    mv[1, 100] = (127, 1)
    curr[1, 100] = prev[2, 227]
    mv[0, 5] = (0, -128)                                  # outside: against 0
    curr[0, 5] = (3, 0, 0, 4)
    sad = pair.sad_map(prev, curr, mv)
    assert sad[1, 200] == 0 and sad[1, 100] == 0 and sad[0, 5] == 7
    rest = prev.astype(np.int64).sum() - prev[1, 200].astype(np.int64).sum() - prev[1, 100].astype(np.int64).sum() - prev[0, 5].astype(np.int64).sum()
    assert pair.pair_stats(prev, curr, mv, 7)[2] == rest + 7
    assert pair.matched_mask(prev, curr, mv, 7)[[1, 1, 0], [200, 100, 5]].all()
    assert not pair.matched_mask(prev, curr, mv, 6)[0, 5]


def test_one_by_one_frame():
    prev, curr = frame(1, 1, (10, 20, 30, 40)), frame(1, 1, (13, 20, 25, 40))
    assert pair.pair_stats(prev, curr, np.zeros((1, 1, 2), np.int8), 8) == (1, 1, 8)
    assert pair.pair_stats(prev, curr, np.zeros((1, 1, 2), np.int8), 7) == (1, 0, 8)
    away = np.array([[(1, 0)]], np.int8)                  # any non-zero vector leaves a 1 x 1 image
    assert pair.pair_stats(prev, curr, away, 97) == (1, 0, 98)
    assert pair.pair_stats(prev, curr, away, 98) == (1, 1, 98)


def test_sad_sum_on_a_constant_pair():
    w, h = 37, 11
    prev, curr = frame(h, w, (0, 0, 0, 0)), frame(h, w, (255, 255, 255, 255))
    mv = np.zeros((h, w, 2), np.int8)
    assert pair.pair_stats(prev, curr, mv, 1019) == (w * h, 0, 1020 * w * h)
    assert pair.pair_stats(prev, curr, mv, 1020) == (w * h, w * h, 1020 * w * h)
    assert pair.pair_stats(curr, prev, mv, 0) == (w * h, 0, 1020 * w * h)
    mv[...] = (w, 0)                                      # every fetch outside: curr against 0
    assert pair.pair_stats(curr, curr, mv, 0) == (w * h, 0, 1020 * w * h)
    assert pair.pair_stats(curr, prev, mv, 0) == (w * h, w * h, 0)


# ---- the separation that the threshold rests on

W, H = 200, 120
SEED_A, SEED_B = synth.BASE_SEED, synth.BASE_SEED + 1


def separation_pairs():
    """(name, prev, curr, is it a cut): the six pairs of DESIGN.md section 4.9."""
    pan_prev = synth.make_prev(W, H)
    pan_curr = synth.translate(pan_prev, (3, -2))
    noisy = np.clip(pan_curr.astype(np.int16) + np.random.default_rng(5).integers(-4, 5, pan_curr.shape), 0, 255).astype(np.uint8)
    return [("matrix_scene", *cases.matrix_scene(W, H), False),
            ("pan(3,-2)", pan_prev, pan_curr, False),
            ("pan(3,-2) + noise of +-4", pan_prev, noisy, False),
            ("still", pan_prev, pan_prev.copy(), False),
            ("cut: synth seed A -> seed B", synth.make_prev(W, H, SEED_A), synth.make_prev(W, H, SEED_B), True),
            ("cut: textured seed 1 -> seed 2", cases.textured(W, H, 1), cases.textured(W, H, 2), True)]


def test_motion_and_cuts_are_far_apart():
    """Matched pixels per thousand at match_sad 48 under the vectors of the three estimators' CPU models: every moving or
    still pair at or above 700, both cuts at or below 50.  The threshold of 500 that the GPU tests use lies between."""
    import oracle
    for name, prev, curr, is_cut in separation_pairs():
        vectors = {"full, reference order": oracle.motion(prev, curr, semantics=0).astype(np.int8),
                   "full, intended order": oracle.motion(prev, curr, semantics=1).astype(np.int8),
                   "pyramid (2, 16, 2)": pm.motion_pyramid(prev, curr, 2, 16, 2)}
        for estimator, mv in vectors.items():
            stats = pair.pair_stats(prev, curr, mv, 48)
            p = pair.permille(stats)
            print(f"{name:34s} {estimator:24s} {p:5d} per thousand, sad_sum {stats[2]}")
            if is_cut:
                assert p <= 50, (name, estimator, p)
            else:
                assert p >= 700, (name, estimator, p)
            assert pair.cut(stats, 500) == is_cut


# ---- the decision's boundary in exact integers

def test_decision_boundary():
    for m in (0, 1, 499, 500, 501, 999, 1000):
        stats = (1000, m, 0)
        assert not pair.cut(stats, m)                     # matched * 1000 == permille * pixels: no cut
        if m < 1000:
            assert pair.cut(stats, m + 1)
        if m > 0:
            assert not pair.cut(stats, m - 1)
    assert not pair.cut((1000, 0, 0), 0)                  # 0 never cuts
    assert not pair.cut((1, 0, 0), 0)
    assert pair.cut((1000, 0, 0), 1)
    assert not pair.cut((1000, 1000, 0), 1000) and pair.cut((1000, 999, 0), 1000)
    # a pixel count that is no multiple of 1000: 7 pixels, 3 matched = 428.57 per thousand
    assert pair.cut((7, 3, 0), 429) and not pair.cut((7, 3, 0), 428)
    # 8K: the products need more than 32 bits
    px = 7680 * 4320
    assert pair.cut((px, px // 2 - 1, 0), 500) and not pair.cut((px, px // 2, 0), 500)


def test_fallback_sources():
    prev, curr = cases.textured(5, 3, 80), cases.textured(5, 3, 81)
    below = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
    outs = pair.fallback(prev, curr, [0.0, 0.3, below, 0.5, 0.9, 1.0])
    assert [o is curr for o in outs] == [False, False, False, True, True, True]
    assert all(o is prev or o is curr for o in outs)
