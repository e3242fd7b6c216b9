"""The overlay model (tests/overlay_model.py) on the CPU: with an all-zero mask it is the compensated model byte for byte; on
the overlay scenes of DESIGN.md section 4.13 the protected route leaves the overlay exact and its surroundings better than the
plain route; where nothing is an overlay it does no harm; and the hand-made cases that the GPU tests also run
(tests/overlay_cases.py) tell every mutant of overlay_model.c from the model.  CPU only."""
import numpy as np
import pytest

from tests import cases
from tests import mc_model as mc
from tests import overlay_cases as oc
from tests import overlay_model as ov
from tests import refine_model as rm

FACTORS = cases.DYADIC_FACTORS + cases.INEXACT_FACTORS + cases.LIMIT_FACTORS


_chains = {}


def chain_vectors(prev, curr, radius):
    """The full search under the reference semantics, then the refinement where radius >= 0; one search per pair."""
    key = (prev.tobytes(), curr.tobytes())
    if key not in _chains:
        _chains[key] = cases.Chain(prev, curr)
    return _chains[key].vectors("full", radius, 0)


# ---- an all-zero mask is lfg_interpolate_compensated

def zero_mask_inputs():
    prev, curr = cases.matrix_scene()
    yield "matrix scene", prev, curr, chain_vectors(prev, curr, -1), 48
    yield ("random field",) + cases.field("random", 64, 48, 7) + (1020,)
    for w, h in ((1, 1), (7, 5)):
        prev, curr = cases.small_scene(w, h, 3)
        yield f"small scene {w}x{h}", prev, curr, chain_vectors(prev, curr, -1), 48


def test_zero_mask_is_the_compensated_model():
    for name, prev, curr, mv, ms in zero_mask_inputs():
        zero = np.zeros(prev.shape[:2], np.uint8)
        for t in FACTORS:
            assert (ov.keys(prev, curr, mv, zero, t, ms) == mc.keys(prev, curr, mv, t, ms)).all(), (name, t)
            got, want = ov.interpolate_masked(prev, curr, mv, zero, t, ms), mc.interpolate_compensated(prev, curr, mv, t, ms)
            assert (got == want).all(), (name, t)


# ---- the overlay scenes

def routes(prev, curr, radius, t=0.5):
    """(the plain route's frame, the protected route's) at match_sad 48 with the mask of tolerance 0."""
    mv = chain_vectors(prev, curr, radius)
    return (mc.interpolate_compensated(prev, curr, mv, t, 48),
            ov.interpolate_masked(prev, curr, mv, ov.static_mask(prev, curr, 0), t, 48))


def overlay_counts(kind, pan, radius, t=0.5):
    prev, curr, truth, on = oc.scene(kind, pan, t)
    around = oc.near(on)
    plain, protected = routes(prev, curr, radius, t)
    counts = tuple(int((oc.wrong(f, truth) & m).sum()) for f in (plain, protected) for m in (on, around))
    print(f"{kind} pan {pan} radius {radius} t {t}: on the overlay {counts[0]} -> {counts[2]} of {int(on.sum())}, "
          f"near it {counts[1]} -> {counts[3]} of {int(around.sum())}")
    return counts


@pytest.mark.parametrize("radius", [-1, 1])
@pytest.mark.parametrize("kind,pan", oc.SCENES)
def test_overlay_scenes(kind, pan, radius):
    _, plain_near, on_overlay, near_it = overlay_counts(kind, pan, radius)
    assert on_overlay == 0
    assert near_it < plain_near


@pytest.mark.parametrize("t", [0.25, 0.75])
def test_glyphs_at_other_factors(t):
    _, plain_near, on_overlay, near_it = overlay_counts("glyphs", (8, -4), -1, t)
    assert on_overlay == 0
    assert near_it < plain_near


# ---- no harm where nothing is an overlay

def test_no_harm_without_an_overlay():
    prev, curr = cases.matrix_scene()
    truth = rm.moving_objects(200, 120, pan=(4, -2), squares=((24, (60, 40), (10, 6)), (32, (120, 56), (-14, 4))))[3]
    truth[76:108, 8:48] = (90, 140, 200, 255)
    inside = oc.interior(prev.shape[:2])
    for name, (prev, curr, truth) in (("matrix scene", (prev, curr, truth)), ("flat moving square", oc.flat_moving_square())):
        plain, protected = routes(prev, curr, -1)
        a, b = int((oc.wrong(plain, truth) & inside).sum()), int((oc.wrong(protected, truth) & inside).sum())
        print(f"{name}: wrong interior pixels {a} -> {b}")
        assert b <= a, name


def test_bare_pan_is_unchanged():
    prev, curr = oc.bare_pan()
    assert not ov.static_mask(prev, curr, 0).any()
    plain, protected = routes(prev, curr, -1)
    assert (plain == protected).all()


# ---- the hand-made cases: what the model says, and that they tell the mutants from it

def test_hand_made_cases_state_the_definition():
    prev, curr, mv, mask, ms = oc.static_under_collision()
    K = ov.keys(prev, curr, mv, mask, 0.5, ms)
    assert K[4, 4] == ov.STATIC and K[4, 5] == mc.key(2, 0)
    out = ov.interpolate_masked(prev, curr, mv, mask, 0.5, ms)
    mix = np.rint((prev[4, 4].astype(np.float64) + curr[4, 4]) / 2)
    assert (np.abs(out[4, 4] - mix) <= 1).all() and (out[4, 5] == prev[4, 6]).all()       # P.x = 6.5: prev's sample alone
    for value in (1, 128):
        assert (ov.interpolate_masked(*oc.static_under_collision(value)[:4], 0.5, ms) == out).all(), value

    prev, curr, mv, mask, ms = oc.walk_past_static_run()
    K = ov.keys(prev, curr, mv, mask, 0.5, ms)
    assert (K[0, :6] == ov.HOLE).all() and (K[0, 6:8] == ov.STATIC).all() and K[0, 8] == mc.key(-4, 0)
    out = ov.interpolate_masked(prev, curr, mv, mask, 0.5, ms)
    assert (out[0, 5] == prev[0, 3]).all()                            # u = (-4, 0): P.x = 3.5, c = 7 static: prev's sample alone

    prev, curr, mv, mask, ms = oc.rule_on_projected_pixels()
    out = ov.interpolate_masked(prev, curr, mv, mask, 0.5, ms)
    assert (out[2, 6] == curr[2, 5]).all() and (out[5, 6] == prev[5, 7]).all()

    prev, curr, mv, mask, ms = oc.rule_on_a_hole(True)
    assert (ov.interpolate_masked(prev, curr, mv, mask, 0.5, ms)[0, 8] == curr[0, 9]).all()
    prev, curr, mv, mask, ms = oc.rule_on_a_hole(False)
    assert (ov.interpolate_masked(prev, curr, mv, mask, 0.5, ms)[0, 8] == prev[0, 6]).all()


def test_the_walk_reaches_16_through_the_call():
    """cases.mc_walk_reach under an all-zero mask: exactly the 65 pixels of the compensated model.  With (26 .. 29, 20) static
    the walk passes over the run: 61, the 65 less the run itself, and the tip (36, 20) still finds (20, 20)."""
    prev, curr, mv, blank = cases.mc_walk_reach()
    ms = cases.WALK_REACH_MATCH_SAD
    for t in cases.WALK_REACH_FACTORS:
        for mask, run in ((np.zeros((40, 40), np.uint8), False), (cases.walk_reach_static_run(), True)):
            K = ov.keys(prev, curr, mv, mask, t, ms)
            assert K[20, 20] == mc.key(2, 0) and (K == ov.STATIC).sum() == (4 if run else 0) and (K == ov.HOLE).sum() == (1595 if run else 1599)
            cases.check_walk_reach(ov.interpolate_masked(prev, curr, mv, mask, t, ms),
                                   ov.interpolate_masked(prev, curr, blank, mask, t, ms), (t, run), static_run=run)


def test_region_of_interest_is_the_crop():
    prev, curr, mv, mask, ms, (x, y, w, h) = oc.region_of_interest()
    crop = tuple(a[y:y + h, x:x + w] for a in (prev, curr, mv, mask))
    whole = ov.interpolate_masked(prev, curr, mv, mask, 0.5, ms)
    assert (ov.interpolate_masked(*crop, 0.5, ms) != whole[y:y + h, x:x + w]).any()         # a call of its own, not a window


@pytest.mark.parametrize("mutant", ov.MUTANTS)
def test_shared_cases_tell_every_mutant_from_the_model(mutant):
    caught = []
    for name, (prev, curr, mv, mask, ms) in oc.hand_made().items():
        for t in FACTORS:
            if (ov.interpolate_masked(prev, curr, mv, mask, t, ms) != ov.interpolate_masked(prev, curr, mv, mask, t, ms, mutant=mutant)).any():
                caught.append(name)
                break
    print(f"{mutant}: caught by {caught}")
    assert caught, mutant


def test_the_stricter_variant_costs_the_flat_square():
    """static pixels that stop projecting leave more of a flat moving object wrong than the model does."""
    prev, curr, truth = oc.flat_moving_square()
    mv, mask, inside = chain_vectors(prev, curr, -1), ov.static_mask(prev, curr, 0), oc.interior(prev.shape[:2])
    model = int((oc.wrong(ov.interpolate_masked(prev, curr, mv, mask, 0.5, 48), truth) & inside).sum())
    strict = int((oc.wrong(ov.interpolate_masked(prev, curr, mv, mask, 0.5, 48, mutant="NO_PROJECT"), truth) & inside).sum())
    print(f"flat moving square: model {model}, static pixels not projecting {strict}")
    assert strict > model
