"""Inputs that tests/test_bidir_model.py (CPU) and tests/test_gpu_bidirectional.py share, so that the two cannot drift apart: the
factors, gates and tolerances of lfg_interpolate_compensated_bidirectional, the vector-field pairs that need no estimator, and
the hand-made cases, each stated through the public inputs alone.  fwd is on curr's grid (prev(q + f) ~ curr(q)), bwd on prev's
(curr(p + b) ~ prev(p))."""
from __future__ import annotations

import numpy as np

from tests import cases

FACTORS = sorted(set(cases.DYADIC_FACTORS + cases.INEXACT_FACTORS + cases.LIMIT_FACTORS + [0.0, 1.0]))
MATCH = (0, 48, 1020)
TOLERANCES = (0, 1, 64)
FIELDS = ("uniform", "piecewise", "random", "small")


def field(kind, w, h, seed):
    """(prev, curr, fwd, bwd): cases.field's frames and forward vectors with a backward field to go with them.
    "uniform": bwd = -fwd everywhere, every interior vector confirmed at tolerance 0.
    "piecewise": bwd = -fwd's quadrants with a third of the vectors off by up to 2 per component: all three tolerances differ.
    "random": independent draws over all 256 byte values, -128 included: nearly nothing is confirmed below tolerance 64.
    "small": independent draws from [-3, 3]^2 on a pair of similar frames: the gate and the check both pass and fail often, on
    images of a few pixels too."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "small":
        prev = cases.textured(w, h, seed)
        curr = np.clip(prev.astype(np.int16) + rng.integers(-8, 9, prev.shape), 0, 255).astype(np.uint8)
        return prev, curr, rng.integers(-3, 4, (h, w, 2)).astype(np.int8), rng.integers(-3, 4, (h, w, 2)).astype(np.int8)
    prev, curr, fwd = cases.field(kind, w, h, seed)
    if kind == "random":
        return prev, curr, fwd, rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
    bwd = (-fwd.astype(np.int16)).astype(np.int8)
    if kind == "piecewise":
        off = rng.integers(-2, 3, (h, w, 2)).astype(np.int8)
        off[rng.random((h, w)) > 1.0 / 3.0] = 0
        bwd = bwd + off
    else:
        assert kind == "uniform", kind
    return prev, curr, fwd, bwd


def flat(w=16, h=16, colour=(90, 140, 200, 255)):
    """Two equal flat frames and zero fields: every vector passes the gate, even at match_sad 0."""
    f = np.empty((h, w, 4), np.uint8)
    f[...] = colour
    return f, f.copy(), np.zeros((h, w, 2), np.int8), np.zeros((h, w, 2), np.int8)


def false_match_on_flat():
    """(prev, curr, fwd, bwd): fwd(8, 8) = (5, 0) passes the gate on the flat frames, and bwd(13, 8) = (0, 0) disagrees with it
    by 5: at t = 0.5 it projects to (11, 8) at tolerance 5 and not at 0 .. 4, where (11, 8) keeps its own (0, 0)."""
    prev, curr, fwd, bwd = flat()
    fwd[8, 8] = (5, 0)
    return prev, curr, fwd, bwd


def crack():
    """(prev, curr, fwd, bwd) of 32 x 8, textured, for match_sad 1020 and t = 0.25: columns 0 .. 15 of curr hold (4, 0) and land
    on 3 .. 18, columns 16 .. 31 hold (5, 0) and land from 20 on: column 19 is a crack, which the hole walk would fill with (4, 0),
    the left region's.  prev's column 20 is the one the step skips; its bwd = (-5, 0) is off by 1 against fwd(15) = (4, 0) and
    lands on 19 carrying (5, 0).  prev's columns up to 19 hold (-4, 0), those from 21 on (-5, 0)."""
    w, h = 32, 8
    prev, curr = cases.textured(w, h, 71), cases.textured(w, h, 72)
    fwd, bwd = np.zeros((h, w, 2), np.int8), np.zeros((h, w, 2), np.int8)
    fwd[:, :16], fwd[:, 16:] = (4, 0), (5, 0)
    bwd[:, :20], bwd[:, 20:] = (-4, 0), (-5, 0)
    return prev, curr, fwd, bwd


def revealed_and_covered():
    """(prev, curr, fwd, bwd, obj): cases.mc_revealed_and_covered with the field measured the other way: an object moves from
    (4, 2) to (6, 2) over black, fwd(6, 2) = (-2, 0), bwd(4, 2) = (2, 0); match_sad 0, tolerance 0."""
    prev, curr, fwd, obj = cases.mc_revealed_and_covered()
    bwd = np.zeros_like(fwd)
    bwd[2, 4] = (2, 0)
    return prev, curr, fwd, bwd, obj


PREV_COLOUR, CURR_COLOUR, MIXED_COLOUR = (100, 50, 200, 255), (200, 150, 0, 255), (150, 100, 100, 255)   # the mix at t = 0.5


def hole_rule(cbad: bool, pbad: bool):
    """(prev, curr, fwd, bwd) of 8 x 8 for the sampling step at t = 0.5, match_sad 1020, tolerance 0, from a key image that is
    key(0, 0) but for a hole at (4, 2): the fill is (0, 0) and c = p = (4, 2).  prev is flat PREV_COLOUR and curr flat CURR_COLOUR.
    cbad: fwd(4, 2) = (1, 0), confirmed by bwd(5, 2) = (-1, 0).  pbad alone: bwd(4, 2) = (1, 0), confirmed by fwd(5, 2) = (-1, 0).
    Both: bwd(4, 2) = (-1, 0), confirmed by fwd(3, 2) = (1, 0) -- it carries (1, 0), which is not the fill either."""
    prev, curr = np.empty((8, 8, 4), np.uint8), np.empty((8, 8, 4), np.uint8)
    prev[...], curr[...] = PREV_COLOUR, CURR_COLOUR
    fwd, bwd = np.zeros((8, 8, 2), np.int8), np.zeros((8, 8, 2), np.int8)
    if cbad:
        fwd[2, 4], bwd[2, 5] = (1, 0), (-1, 0)
    if pbad and not cbad:
        bwd[2, 4], fwd[2, 5] = (1, 0), (-1, 0)
    if pbad and cbad:
        bwd[2, 4], fwd[2, 3] = (-1, 0), (1, 0)
    return prev, curr, fwd, bwd


def minus_128():
    """(prev, curr, fwd, bwd) of 160 x 2, textured, for match_sad 1020, tolerance 1 and t = 0.5: bwd(130, 0) = (-128, 0) points at
    (2, 0), whose fwd = (127, 0) is off by 1: everything but the -128 rule confirms it, and carried as (127, 0) it would land on
    (66, 0) and win there over (66, 0)'s own (0, 0)."""
    w, h = 160, 2
    prev, curr = cases.textured(w, h, 81), cases.textured(w, h, 82)
    fwd, bwd = np.zeros((h, w, 2), np.int8), np.zeros((h, w, 2), np.int8)
    bwd[0, 130] = (-128, 0)
    fwd[0, 2] = (127, 0)
    return prev, curr, fwd, bwd


def tolerance_edges():
    """(prev, curr, fwd, bwd, {(x, y): (L1 distance, Chebyshev distance)}) of 16 x 8, textured, for match_sad 1020: four forward
    vectors on row 2 whose far ends disagree with them by a known amount; every other vector is (0, 0) both ways."""
    w, h = 16, 8
    prev, curr = cases.textured(w, h, 91), cases.textured(w, h, 92)
    fwd, bwd = np.zeros((h, w, 2), np.int8), np.zeros((h, w, 2), np.int8)
    fwd[2, 1], bwd[4, 3] = (2, 2), (-1, -1)           # L1 2, Chebyshev 1
    fwd[2, 5], bwd[2, 6] = (1, 0), (0, 0)             # L1 1, Chebyshev 1
    fwd[2, 9], bwd[5, 9] = (0, 3), (-2, -4)           # L1 3, Chebyshev 2
    fwd[2, 13], bwd[1, 12] = (-1, -1), (1, 1)         # exact
    return prev, curr, fwd, bwd, {(1, 2): (2, 1), (5, 2): (1, 1), (9, 2): (3, 2), (13, 2): (0, 0)}


def walk_reach():
    """(prev, curr, fwd, bwd, blank): cases.mc_walk_reach with the field measured the other way, for match_sad 1020 and tolerance
    0.  bwd is (127, 0) everywhere but bwd(21, 20) = (-2, 0): it confirms fwd(19, 20) = (2, 0), is confirmed by it, and lands on
    (20, 20) as well at t = 0.5 and 0.3 (floor(-2 * 0.5 + 0.5) = floor(-2 * 0.3 + 0.5) = -1), carrying (2, 0).  No (127, 0) is
    confirmed: its far end is outside the image.  `blank` is (127, 0) everywhere, for both fields: K all holes."""
    prev, curr, fwd, blank = cases.mc_walk_reach()
    bwd = blank.copy()
    bwd[20, 21] = (-2, 0)
    return prev, curr, fwd, bwd, blank


def shared_cases():
    """(name, prev, curr, fwd, bwd, match_sad, tolerances): the hand-made cases through the public call, on the CPU and the GPU."""
    yield ("false_match", *false_match_on_flat(), 0, (0, 4, 5))
    yield ("crack", *crack(), 1020, (0, 1))
    yield ("revealed_and_covered", *revealed_and_covered()[:4], 0, (0, 1))
    yield ("minus_128", *minus_128(), 1020, (0, 1, 2))
    yield ("tolerance_edges", *tolerance_edges()[:4], 1020, (0, 1, 2, 3))
    for cbad in (False, True):
        for pbad in (False, True):
            yield (f"hole_rule_{int(cbad)}{int(pbad)}", *hole_rule(cbad, pbad), 1020, (0,))
