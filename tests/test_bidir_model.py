"""Known answers for the CPU model of lfg_interpolate_compensated_bidirectional and lfg_motion_consistency
(tests/bidir_model.py): both limits, a uniform pan against the one-field model, one hand-worked case per changed rule of the
header's definition, and the model's mutants against the cases that the GPU tests share (tests/bidir_cases.py)."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import bidir_cases as bc
from tests import bidir_model as bd
from tests import cases
from tests import mc_model as mc

HOLE, key = bd.HOLE, mc.key


def numpy_consistency(a, b, tolerance):
    """lfg_motion_consistency's definition again, in numpy."""
    h, w = a.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    rx, ry = xs + a[..., 0].astype(int), ys + a[..., 1].astype(int)
    inside = (rx >= 0) & (rx < w) & (ry >= 0) & (ry < h)
    other = b[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)].astype(int)
    l1 = np.abs(a.astype(int) + other).sum(-1)
    return np.where(inside & (l1 <= tolerance), 255, 0).astype(np.uint8)


@pytest.mark.parametrize("kind", bc.FIELDS)
def test_consistency_is_the_definition(kind):
    for w, h, seed in ((1, 1, 1), (7, 5, 2), (50, 40, 3)):
        _, _, fwd, bwd = bc.field(kind, w, h, seed)
        for tol in bc.TOLERANCES:
            assert (bd.consistency(fwd, bwd, tol) == numpy_consistency(fwd, bwd, tol)).all(), (kind, w, h, tol)
            assert (bd.consistency(bwd, fwd, tol) == numpy_consistency(bwd, fwd, tol)).all(), (kind, w, h, tol)
    _, _, fwd, bwd = bc.field("piecewise", 50, 40, 3)                 # the three tolerances are three masks
    counts = [int((bd.consistency(fwd, bwd, tol) == 255).sum()) for tol in bc.TOLERANCES]
    assert 0 < counts[0] < counts[1] < counts[2], counts


@pytest.mark.parametrize("match_sad", bc.MATCH)
@pytest.mark.parametrize("tolerance", bc.TOLERANCES)
def test_t0_gives_prev_and_t1_gives_curr(match_sad, tolerance):
    confirmed = 0
    for kind in ("random", "small", "piecewise"):
        for w, h, seed in ((1, 1, 1), (7, 5, 2), (50, 40, 3)):
            prev, curr, fwd, bwd = bc.field(kind, w, h, seed)
            if kind == "random":
                fwd[0, 0] = bwd[h - 1, w - 1] = (-128, -128)
            assert (bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.0, match_sad, tolerance) == prev).all(), (kind, w, h)
            assert (bd.interpolate_bidirectional(prev, curr, fwd, bwd, 1.0, match_sad, tolerance) == curr).all(), (kind, w, h)
            confirmed += int((bd.keys(prev, curr, fwd, bwd, 0.0, match_sad, tolerance) != HOLE).sum())
    assert match_sad == 0 or confirmed > 0                            # the limits are no accident of empty key images


def test_uniform_pan_equals_the_one_field_model_on_the_interior():
    prev = synth.make_prev(96, 64)
    curr = synth.translate(prev, (6, -4))
    fwd = np.zeros((64, 96, 2), np.int8)
    fwd[...] = (-6, 4)
    bwd = (-fwd.astype(np.int16)).astype(np.int8)
    for t in (0.25, 0.5, 0.3, 0.9):
        got = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, 48, 0)
        want = mc.interpolate_compensated(prev, curr, fwd, t, 48)
        assert (got[16:-16, 16:-16] == want[16:-16, 16:-16]).all(), t
    assert (bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.5, 48, 0)[16:-16, 16:-16]
            == synth.translate(prev, (3, -2))[16:-16, 16:-16]).all()


def test_a_false_match_on_a_flat_area_does_not_project():
    prev, curr, fwd, bwd = bc.false_match_on_flat()
    assert mc.keys(prev, curr, fwd, 0.5, 0)[8, 11] == key(5, 0)       # the gate alone lets it through
    for tol in range(0, 5):
        K = bd.keys(prev, curr, fwd, bwd, 0.5, 0, tol)
        assert K[8, 11] == key(0, 0) and (K[K != HOLE] == key(0, 0)).all(), tol
        assert K[8, 8] == HOLE and (K == HOLE).sum() == 1             # prev's (8, 8) points at a vector that is not its own
    assert bd.keys(prev, curr, fwd, bwd, 0.5, 0, 5)[8, 11] == key(5, 0)
    assert bd.keys(prev, curr, fwd, bwd, 0.5, 0, 5, "backward")[8, 11] == key(0, 0)


def test_the_backward_projection_fills_a_crack_with_the_measured_vector():
    prev, curr, fwd, bwd = bc.crack()
    t = 0.25
    one = mc.keys(prev, curr, fwd, t, 1020)
    assert (one[:, 19] == HOLE).all() and (one[:, 18] == key(4, 0)).all() and (one[:, 20] == key(5, 0)).all()
    # ... which the one-field model fills with the left region's vector, the shorter one, and calls covered: prev alone at
    # P = 19.5 + 4 * 0.25, a texel centre
    assert (mc.interpolate_compensated(prev, curr, fwd, t, 1020)[:, 19] == prev[:, 20]).all()
    forward = bd.keys(prev, curr, fwd, bwd, t, 1020, 1, "forward")
    assert (forward[:, 19] == HOLE).all()
    assert (bd.keys(prev, curr, fwd, bwd, t, 1020, 1, "backward")[:, 19] == key(5, 0)).all()
    both = bd.keys(prev, curr, fwd, bwd, t, 1020, 1)
    assert (both[:, 19] == key(5, 0)).all() and (both[:, 3:31] != HOLE).all()     # (curr's 27 on point outside prev)
    assert (bd.keys(prev, curr, fwd, bwd, t, 1020, 0)[:, 19] == HOLE).all()      # prev's column 20 is off by 1
    measured = forward.copy()
    measured[:, 19] = key(5, 0)
    got = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, 1020, 1)
    assert (got[:, 16:24] == bd.sample(prev, curr, fwd, bwd, measured, t, 1020, 1)[:, 16:24]).all()
    assert not (got[:, 19] == mc.interpolate_compensated(prev, curr, fwd, t, 1020)[:, 19]).all()


def test_the_walk_reaches_16_through_the_call():
    """bc.walk_reach: both projections land on (20, 20), the only word of K, and change exactly the holes within 16 steps."""
    prev, curr, fwd, bwd, blank = bc.walk_reach()
    ms = cases.WALK_REACH_MATCH_SAD
    for t in cases.WALK_REACH_FACTORS:
        for direction in ("forward", "backward", "both"):
            K = bd.keys(prev, curr, fwd, bwd, t, ms, 0, direction)
            assert K[20, 20] == key(2, 0) and (K != HOLE).sum() == 1, (t, direction)
        assert (bd.keys(prev, curr, blank, blank, t, ms, 0) == HOLE).all(), t
        cases.check_walk_reach(bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, 0),
                               bd.interpolate_bidirectional(prev, curr, blank, blank, t, ms, 0), t)


def test_revealed_and_covered_through_the_call():
    prev, curr, fwd, bwd, obj = bc.revealed_and_covered()
    K = bd.keys(prev, curr, fwd, bwd, 0.5, 0, 0)
    assert K[2, 5] == key(-2, 0) and K[2, 4] == HOLE and K[2, 6] == HOLE and (K != HOLE).sum() == 62
    assert bd.keys(prev, curr, fwd, bwd, 0.5, 0, 0, "backward")[2, 5] == key(-2, 0)     # prev's object carries -b
    out = bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.5, 0, 0)
    want = np.zeros_like(prev)
    want[2, 5] = obj                                                  # half way; (4, 2) revealed and (6, 2) covered: both black
    assert (out == want).all()


@pytest.mark.parametrize("cbad, pbad, colour", [(True, False, bc.PREV_COLOUR), (False, True, bc.CURR_COLOUR),
                                                (True, True, bc.MIXED_COLOUR), (False, False, bc.MIXED_COLOUR)])
def test_the_hole_rule_asks_both_frames(cbad, pbad, colour):
    prev, curr, fwd, bwd = bc.hole_rule(cbad, pbad)
    K = np.full((8, 8), key(0, 0), np.uint32)
    K[2, 4] = HOLE
    out = bd.sample(prev, curr, fwd, bwd, K, 0.5, 1020, 0)
    assert tuple(out[2, 4]) == colour
    assert all(tuple(out[y, x]) == bc.MIXED_COLOUR for y in range(8) for x in range(8) if (x, y) != (4, 2))
    # a vector that the other field does not confirm is not "other content": the one-field rule would call (4, 2) covered
    if cbad and not pbad:
        bwd[2, 5] = (0, 0)
        assert tuple(bd.sample(prev, curr, fwd, bwd, K, 0.5, 1020, 0)[2, 4]) == bc.MIXED_COLOUR
        assert tuple(mc.sample(prev, curr, fwd, K, 0.5, 1020)[2, 4]) == bc.PREV_COLOUR


def test_minus_128_is_refused_on_prevs_grid_only():
    prev, curr, fwd, bwd = bc.minus_128()
    assert bd.consistency(bwd, fwd, 1)[0, 130] == 255                  # the vector half alone passes it
    for t in (0.5, 0.25):
        K = bd.keys(prev, curr, fwd, bwd, t, 1020, 1)
        assert (K[K != HOLE] == key(0, 0)).all()
    assert bd.keys(prev, curr, fwd, bwd, 0.5, 1020, 1, mutant="NEG128_AS_127")[0, 66] == key(127, 0)
    assert not (bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.5, 1020, 1)
                == bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.5, 1020, 1, mutant="NEG128_AS_127")).all()
    # on curr's grid -128 is a vector like any other, in fwd and in the bwd it is checked against
    prev, curr, fwd, bwd = bc.flat(160, 2)
    fwd[0, 130], bwd[0, 2] = (-128, 0), (127, 0)
    assert bd.keys(prev, curr, fwd, bwd, 0.5, 0, 1, "forward")[0, 66] == key(-128, 0)
    fwd[0, 130], bwd[0, 3] = (-127, 0), (-128, 0)
    assert bd.keys(prev, curr, fwd, bwd, 0.5, 0, 64, "forward")[0, 67] == key(0, 0)     # |-127 - 128| = 255


def test_the_tolerance_is_l1_and_inclusive():
    prev, curr, fwd, bwd, distances = bc.tolerance_edges()
    for tol in (0, 1, 2, 3):
        mask = bd.consistency(fwd, bwd, tol)
        for (x, y), (l1, _) in distances.items():
            assert (mask[y, x] == 255) == (l1 <= tol), (x, y, tol)
    assert bd.consistency(fwd, bwd, 1, mutant="CHEBYSHEV")[2, 1] == 255 and bd.consistency(fwd, bwd, 1)[2, 1] == 0
    assert bd.consistency(fwd, bwd, 1, mutant="STRICT")[2, 5] == 0 and bd.consistency(fwd, bwd, 1)[2, 5] == 255
    assert bd.consistency(fwd, bwd, 0, mutant="STRICT").max() == 0 and bd.consistency(fwd, bwd, 0)[2, 13] == 255


@pytest.mark.parametrize("mutant", bd.MUTANTS)
def test_the_shared_cases_tell_the_mutants_from_the_model(mutant):
    """What test_gpu_bidirectional.py runs byte for byte: a kernel with one of these mistakes fails there."""
    told = []
    for name, prev, curr, fwd, bwd, ms, tols in bc.shared_cases():
        for tol in tols:
            for t in (0.25, 0.5):
                if not (bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol)
                        == bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol, mutant=mutant)).all():
                    told.append((name, tol, t))
    print(mutant, told)
    assert told


def test_roi_equals_the_whole_frame():
    prev, curr, fwd, bwd = bc.field("small", 70, 50, 5)
    whole = bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.3, 48, 1)
    for x, y, w, h in ((0, 0, 16, 16), (54, 34, 16, 16), (20, 10, 33, 7)):
        assert (bd.interpolate_bidirectional(prev, curr, fwd, bwd, 0.3, 48, 1, roi=(x, y, w, h)) == whole[y:y + h, x:x + w]).all()


@pytest.mark.parametrize("w, h", [(96, 64), (200, 120)])
def test_held_out_pan(w, h):
    """The rows of DESIGN.md section 4.17: a pan of (3, -2) per frame, the pair is frames 0 and 2 and frame 1 is held out; both
    fields from the estimators' CPU models.  The figures are printed, not asserted: inside the border the pan brings in, the
    frame is frame 1 byte for byte under the full search, as under the one-field route."""
    f0 = synth.make_prev(w, h, synth.BASE_SEED)
    f1 = synth.translate(f0, (3, -2), synth.BASE_SEED)
    f2 = synth.translate(f1, (3, -2), synth.BASE_SEED)
    forward, backward = cases.Chain(f0, f2), cases.Chain(f2, f0)
    for estimator in cases.ESTIMATORS:
        fwd, bwd = forward.vectors(estimator, -1, 1), backward.vectors(estimator, -1, 1)
        one = mc.interpolate_compensated(f0, f2, fwd, 0.5)
        rows = {"one field": one}
        for tol in (0, 1, 2):
            rows[f"tolerance {tol}"] = bd.interpolate_bidirectional(f0, f2, fwd, bwd, 0.5, 48, tol)
        for name, frame in rows.items():
            mse = ((frame[..., :3].astype(np.float64) - f1[..., :3]) ** 2).mean()
            psnr = float("inf") if mse == 0 else 10 * np.log10(65025 / mse)
            print(f"{w}x{h} {estimator} {name}: PSNR {psnr:.2f} dB, {int((frame != f1).any(-1).sum())} differing px")
        if estimator == "full":
            b = 32                                                    # search radius 16 + half a block + the pair's (6, -4), both ways
            assert all((frame[b:-b, b:-b] == f1[b:-b, b:-b]).all() for frame in rows.values())
