"""Known answers for the CPU model of lfg_motion_refine (tests/refine_model.py): a uniform field, candidates only, a straight
edge between two motions, the tie order, the image's edges and a 1 x 1 frame."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import cases
from tests import refine_model as rm

RADII = [0, 1, 2]


# The hand-made inputs are built in tests/cases.py: test_gpu_refine.py runs them on the GPU.
textured, warp = cases.textured, cases.warp


def test_offsets_are_the_17_positions():
    assert len(rm.OFFSETS) == len(set(rm.OFFSETS)) == 17
    assert rm.OFFSETS[0] == (0, 0)
    assert {max(abs(dx), abs(dy)) for dx, dy in rm.OFFSETS[1:]} == {4, 8}


@pytest.mark.parametrize("radius", RADII)
def test_uniform_field_is_returned_unchanged(radius):
    w, h = 45, 29
    prev = synth.make_prev(w, h)
    for v, curr in (((5, -3), synth.translate(prev, (-5, 3))), ((-128, 127), textured(w, h, 2)), ((0, 0), textured(w, h, 3))):
        mv = np.zeros((h, w, 2), np.int8)
        mv[...] = v
        assert (rm.refine(prev, curr, mv, radius) == mv).all(), (v, radius)


@pytest.mark.parametrize("radius", RADII)
def test_every_output_is_one_of_its_candidates(radius):
    w, h = 37, 23
    rng = np.random.default_rng(radius)
    prev, curr = textured(w, h, 10), textured(w, h, 11)
    mv = rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
    out = rm.refine(prev, curr, mv, radius)
    for y in range(h):
        for x in range(w):
            assert tuple(int(c) for c in out[y, x]) in rm.candidates(mv, x, y), (x, y)
    # and the minimum of the key over them (a direct restatement for a few pixels)
    for x, y in ((0, 0), (w - 1, h - 1), (18, 11), (3, 20)):
        def cost(v):
            s = 0
            for ry in range(y - radius, y + radius + 1):
                for rx in range(x - radius, x + radius + 1):
                    if 0 <= rx < w and 0 <= ry < h:
                        px, py = rx + v[0], ry + v[1]
                        p = prev[py, px].astype(int) if 0 <= px < w and 0 <= py < h else np.zeros(4, int)
                        s += int(np.abs(curr[ry, rx].astype(int) - p).sum())
            return s
        want = min(rm.candidates(mv, x, y), key=lambda v: (cost(v), v[0] ** 2 + v[1] ** 2, v[1], v[0]))
        assert tuple(int(c) for c in out[y, x]) == want, (x, y)


def test_roi_equals_whole_frame():
    w, h = 70, 50
    rng = np.random.default_rng(4)
    prev, curr = textured(w, h, 12), textured(w, h, 13)
    mv = rng.integers(-20, 21, (h, w, 2)).astype(np.int8)
    for radius in RADII:
        whole = rm.refine(prev, curr, mv, radius)
        for x, y, rw, rh in ((0, 0, 9, 7), (61, 43, 9, 7), (20, 17, 30, 12)):
            assert (rm.refine(prev, curr, mv, radius, roi=(x, y, rw, rh)) == whole[y:y + rh, x:x + rw]).all()


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("vertical", [True, False])
def test_straight_edge_between_two_motions(radius, vertical):
    """Two regions with their own vectors, split by a straight line; the input field has the block matcher's error, a 3 px
    band past the edge holding the other side's vector.  Every pixel comes out with its own region's vector."""
    prev, curr, mv, truth = cases.refine_straight_edge(radius, vertical)
    got = rm.refine(prev, curr, mv, radius)
    bad = np.argwhere((got != truth).any(-1))
    assert len(bad) == 0, bad[:5].tolist()
    assert (mv != truth).any()                     # the input was wrong in the band


@pytest.mark.parametrize("radius", RADII)
def test_ties_go_to_shorter_then_smaller_vy_then_smaller_vx(radius):
    for vectors, want in cases.REFINE_TIES:
        prev, curr, mv = cases.refine_tie_case(vectors)
        assert tuple(int(c) for c in rm.refine(prev, curr, mv, radius)[8, 8]) == want, vectors


def test_cost_comes_before_length():
    prev, curr, mv = cases.refine_cost_before_length()   # (6, 2) at (16, 8): a candidate of (12, 8) and of (8, 8)
    got = rm.refine(prev, curr, mv, 1)
    assert tuple(got[8, 12]) == (6, 2) and tuple(got[8, 8]) == (6, 2)
    assert tuple(got[8, 16]) == (6, 2)
    assert tuple(got[0, 0]) == (0, 0)


@pytest.mark.parametrize("radius", RADII)
def test_candidates_outside_the_image_are_skipped(radius):
    """A 4 x 1 frame: pixel 0's only candidate is its own (x = 4 and x = 8 are outside), even though (0, 0) would fit
    better; an outside position read as (0, 0) would win here."""
    prev, curr, mv = cases.refine_candidates_outside()
    got = rm.refine(prev, curr, mv, radius)
    assert tuple(got[0, 0]) == (2, 0)
    assert tuple(got[0, 1]) == (0, 0) and tuple(got[0, 3]) == (0, 0)   # pixel 0 is none of theirs either (offsets 4 and 8)


@pytest.mark.parametrize("radius", RADII)
def test_prev_outside_the_image_reads_as_zero(radius):
    """curr is 0 and prev 255: a vector that moves the whole window out of the image costs 0 and beats (0, 0), which costs
    255 per channel.  With prev clamped to the edge both would cost the same and (0, 0) would win on length."""
    prev, curr, mv = cases.refine_prev_outside_zero()
    got = rm.refine(prev, curr, mv, radius)
    for x, y in ((6, 6), (2, 6), (10, 6), (6, 2), (2, 2), (6, 10)):
        assert tuple(got[y, x]) == (100, 0), (x, y)
    assert tuple(got[0, 0]) == (0, 0)              # not a candidate of (0, 0): offset (6, 6) is none of the 17


@pytest.mark.parametrize("radius", RADII)
def test_one_by_one_frame(radius):
    prev, curr = textured(1, 1, 50), textured(1, 1, 51)
    for v in ((0, 0), (-128, 127), (3, -7)):
        mv = np.array([[v]], np.int8)
        assert tuple(rm.refine(prev, curr, mv, radius)[0, 0]) == v
