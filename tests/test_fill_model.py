"""The fill plane's CPU model (tests/fill_model.py) held to the existing models at reach 16, to the scene that the reach was
measured on, and to its definition at the edges; and the mutants of fill_model.c told apart by those edge cases."""
import numpy as np
import pytest

from tests import bidir_model as bd, cases, fill_cases as fc, fill_model as fm, mc_model as mc, overlay_model as ov
from tests import pyramid_model
from tests.c_model import HOLE, key

FACTORS = (0.5, 0.25)


def walk16(K, pass_static):
    """The hole walk of compensated_model.h (fill_vector) and overlay_model.c (fill_vector_past_static), restated: (H, W, 2)
    vectors, computed at every pixel."""
    H, W = K.shape
    out = np.zeros((H, W, 2), np.int32)
    for y in range(H):
        for x in range(W):
            best = HOLE
            for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                for j in range(1, 17):
                    nx, ny = x + sx * j, y + sy * j
                    if not (0 <= nx < W and 0 <= ny < H):
                        break
                    word = int(K[ny, nx])
                    if word == HOLE or (pass_static and word == fm.STATIC):
                        continue
                    best = min(best, ((65535 - (word >> 16)) << 16) | (word & 0xFFFF))
                    break
            if best != HOLE:
                out[y, x] = ((best & 0xFF) - 128, ((best >> 8) & 0xFF) - 128)
    return out


@pytest.mark.parametrize("case", list(fc.equivalence_cases()), ids=lambda c: c[0])
def test_reach_16_is_the_walk(case):
    """At reach 16 the plane decodes, at every hole, to the walk's vector, and the three sampled frames are mc_model's,
    overlay_model's and bidir_model's byte for byte."""
    name, prev, curr, fwd, bwd, mask, match_sad, tolerance = case
    if mask is None:
        mask = ov.static_mask(prev, curr, 0)
    for t in FACTORS:
        K = mc.keys(prev, curr, fwd, t, match_sad)
        assert (fm.decoded(fm.plane(K, 16))[K == HOLE] == walk16(K, False)[K == HOLE]).all(), (name, t)
        assert (fm.interpolate_compensated(prev, curr, fwd, t, 16, match_sad) ==
                mc.interpolate_compensated(prev, curr, fwd, t, match_sad)).all(), (name, t)
        Km = ov.keys(prev, curr, fwd, mask, t, match_sad)
        assert (fm.decoded(fm.plane(Km, 16, True))[Km == HOLE] == walk16(Km, True)[Km == HOLE]).all(), (name, t, "masked")
        assert (fm.interpolate_masked(prev, curr, fwd, mask, t, 16, match_sad) ==
                ov.interpolate_masked(prev, curr, fwd, mask, t, match_sad)).all(), (name, t, "masked")
        assert (fm.interpolate_bidirectional(prev, curr, fwd, bwd, t, 16, match_sad, tolerance) ==
                bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, match_sad, tolerance)).all(), (name, t, "bidirectional")


def test_walk_reach_plus_through_the_plane():
    """cases.mc_walk_reach: K is one word at (20, 20); the plane at reach 16 is its vector on cases.walk_reach_plus() but for
    (20, 20) itself, which has no donor, and the hole word everywhere else; at reach 17 the arms are one longer."""
    prev, curr, mv, blank = cases.mc_walk_reach()
    for t in cases.WALK_REACH_FACTORS:
        K = mc.keys(prev, curr, mv, t, cases.WALK_REACH_MATCH_SAD)
        assert (K != HOLE).sum() == 1 and K[20, 20] == key(2, 0)
        want = cases.walk_reach_plus()
        want[20, 20] = False
        P = fm.plane(K, 16)
        assert ((P != HOLE) == want).all() and (P[want] == fm.order(2, 0)).all()
        assert (fm.plane(K, 17) != HOLE).sum() == want.sum() + 4
        assert (fm.plane(mc.keys(prev, curr, blank, t, cases.WALK_REACH_MATCH_SAD), 255) == HOLE).all()


# ---- scene B: what the reach is for

@pytest.fixture(scope="module")
def scene_b():
    (prev, truth, curr), field = fm.fast_scene(**fm.SCENE_B)
    return prev, truth, curr, field, pyramid_model.motion_pyramid(prev, curr)


def test_scene_b_is_the_measured_scene(scene_b):
    """The untouched mc_model on scene B: 2,491 holes of 15,360 pixels with the true field, 97 wrong pixels with it and 496
    with the pyramid's vectors at its defaults."""
    prev, truth, curr, field, pyramid = scene_b
    assert prev.shape == (96, 160, 4)
    assert (mc.keys(prev, curr, field, 0.5, 48) == HOLE).sum() == 2491
    assert fm.wrong_pixels(mc.interpolate_compensated(prev, curr, field, 0.5, 48), truth) == 97
    assert fm.wrong_pixels(mc.interpolate_compensated(prev, curr, pyramid, 0.5, 48), truth) == 496


def test_scene_b_true_field(scene_b):
    prev, truth, curr, field, _ = scene_b
    wrong = {r: fm.wrong_pixels(fm.interpolate_compensated(prev, curr, field, 0.5, r, 48), truth) for r in (16, 32, 255)}
    print("scene B, true field, wrong pixels by reach:", wrong)
    assert wrong[16] == 97 and wrong[32] <= 1 and wrong[255] <= 1, wrong


def test_scene_b_pyramid_vectors(scene_b):
    prev, truth, curr, _, pyramid = scene_b
    wrong = {r: fm.wrong_pixels(fm.interpolate_compensated(prev, curr, pyramid, 0.5, r, 48), truth) for r in (16, 32)}
    print("scene B, pyramid vectors, wrong pixels by reach:", wrong)
    assert wrong[16] == 496 and wrong[32] <= 1, wrong


# ---- the plane at its edges.  Each case is (name, K, reach, pass_static, the plane it must give[, where: the pixels the case is
# about, every pixel if it is left out]).

def _arms(w, h, at, reach, word):
    want = fc.holes(w, h)
    x, y = at
    want[y, max(x - reach, 0):x + reach + 1] = word
    want[max(y - reach, 0):y + reach + 1, x] = word
    want[y, x] = HOLE
    return want


def edge_cases():
    yield "all holes", fc.holes(70, 40), 255, False, fc.holes(70, 40)
    full = np.full((9, 12), key(3, 1), np.uint32)
    yield "no holes", full, 16, False, np.full((9, 12), fm.order(3, 1), np.uint32)
    for reach in (1, 16, 17, 255):                          # one donor: arms of exactly `reach` in an image just large enough
        n, c = 2 * reach + 5, reach + 2
        yield f"one donor, reach {reach}", fc.cross(n, n + 2, (c, c + 1)), reach, False, _arms(n, n + 2, (c, c + 1), reach, fm.order(5, -3))
    # the donor in the corner: (0, 0) sees it from distance 16 along the row and the column of the image's edge, not from 17
    yield "kept at the reach, at the edge", fc.cross(40, 40, (16, 0)), 16, False, _arms(40, 40, (16, 0), 16, fm.order(5, -3))
    yield "dropped past the reach, at the edge", fc.cross(40, 40, (17, 0)), 16, False, _arms(40, 40, (17, 0), 16, fm.order(5, -3))
    # ties between directions: four donors at distance 2 and 3 with |v|^2 = 25 -- the smallest vy wins, then the smallest vx
    K = fc.holes(9, 9)
    K[4, 2], K[4, 6], K[1, 4], K[7, 4] = key(3, 4), key(4, 3), key(-4, 3), key(5, 0)
    only = np.zeros((9, 9), bool)
    only[4, 4] = True
    yield "ties by (vy, vx)", K.copy(), 16, False, np.full((9, 9), fm.order(5, 0), np.uint32), only
    K[7, 4] = HOLE
    yield "ties by vx", K, 16, False, np.full((9, 9), fm.order(-4, 3), np.uint32), only
    # two donors in a row: each pixel takes the nearest of each side, and of those the smaller; a donor sees the other one
    K = fc.holes(9, 3)
    K[1, 2], K[1, 6] = key(3, 4), key(4, 3)
    a, b = fm.order(3, 4), fm.order(4, 3)                   # b < a: vy 3 < 4
    want = fc.holes(9, 3)
    want[1, :] = [a, a, b, b, b, b, a, b, b]
    want[0, 2] = want[2, 2] = a
    want[0, 6] = want[2, 6] = b
    yield "the nearest of each side, then the smaller", K, 16, False, want
    # the longest vector wins a projection and loses a fill: the order is the walk's, not the stored key's
    K = fc.holes(9, 1)
    K[0, 2], K[0, 6] = key(1, 0), key(20, 0)
    want = fc.holes(9, 1)
    want[0, :] = fm.order(1, 0)                             # 0, 1 see the donor at 2 alone; 3 .. 5 see both; 6 sees the one at 2
    want[0, 2] = want[0, 7:] = fm.order(20, 0)              # 2 sees the one at 6, and so do 7 and 8: theirs is the nearest on its side
    yield "walk order, not projection order", K, 16, False, want
    # a static run between hole and donor: passed with pass_static, a donor without it
    K = fc.holes(12, 1)
    K[0, 8] = key(2, 0)
    K[0, 4:7] = fm.STATIC
    passed = fc.holes(12, 1)
    passed[0, :] = fm.order(2, 0)
    passed[0, 8] = HOLE
    yield "a static run is passed", K, 16, True, passed
    S, o = 0xFFFF0000, fm.order(2, 0)                       # the static word in the walk's order: longer than any vector
    stops = np.array([[S, S, S, S, S, S, o, o, S, o, o, o]], np.uint32)
    yield "a static run is a donor without pass_static", K, 16, False, stops
    # the column pass scans K: a donor that only the row pass saw must not travel down the column
    K = fc.holes(5, 5)
    K[0, 0] = key(7, 0)
    want = fc.holes(5, 5)
    want[0, 1:] = want[1:, 0] = fm.order(7, 0)
    yield "no diagonal", K, 16, False, want


EDGE_CASES = [c if len(c) == 6 else c + (np.ones(c[1].shape, bool),) for c in edge_cases()]


def _differs(case, mutant=None):
    name, K, reach, pass_static, want, where = case
    got = fm.plane(K, reach, pass_static, mutant)
    return np.argwhere((got != want) & where)


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c[0])
def test_plane_edge_case(case):
    bad = _differs(case)
    assert len(bad) == 0, (case[0], bad[:4].tolist())


@pytest.mark.parametrize("mutant", fm.MUTANTS)
def test_edge_cases_tell_the_mutant(mutant):
    told = next((case[0] for case in EDGE_CASES if len(_differs(case, mutant))), None)
    print(mutant, "is told apart by:", told)
    assert told, mutant


def test_crafted_patterns_are_what_they_say():
    """fill_cases.py: the cross's arms end on the first pixel behind a seam, and the seam pattern holds its donors."""
    K = fc.cross_at_seams(300, 260, 17)
    (y,), (x,) = np.nonzero((K != HOLE).any(1)), np.nonzero((K != HOLE).any(0))
    assert (x + 17) % fc.LANE_ROW_PIXELS == 0 and (y + 17) % fc.BAND == 0
    P = fm.plane(K, 17)
    assert P[y, x + 17] != HOLE and P[y, x + 18] == HOLE and P[y + 17, x] != HOLE and P[y + 18, x] == HOLE
    S = fc.seams(300, 260, 65)
    assert (S != HOLE).sum() == 12          # seams at 64, 128, 192, 256 both ways: -1 and 320 are outside, the other six are in
