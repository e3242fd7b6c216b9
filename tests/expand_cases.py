"""Hand-made inputs of lfg_motion_expand that the CPU test of the model (tests/test_expand_model.py) and the GPU test
(tests/test_gpu_expand.py) share.  Each case is stated through the public inputs alone and names the departure from the
definition (a mutant of tests/expand_model.c) that it tells from the model, with the pixel and the vector that tell it.

CASES[name]() gives (prev, curr, mv_low, (x, y), want, mutant): the expanded field holds `want` at pixel (x, y) at every
radius, and `mutant` does not."""
from __future__ import annotations

import numpy as np

from tests.cases import textured, warp


def _uniform(w, h, v):
    f = np.zeros((h, w, 2), np.int8)
    f[...] = v
    return f


def saturation():
    """-128 and 127 double to -127 and 127.  Every candidate reads prev outside the 20 x 12 image, so all costs tie and the
    shortest of (-127, 127) + [-1, 1]^2 wins.  Doubling in the byte gives (0, -2) instead."""
    w, h = 20, 12
    return textured(w, h, 1), textured(w, h, 2), _uniform(10, 6, (-128, 127)), (7, 5), (-126, 126), "NO_SATURATION"


def parity():
    """curr(q) = prev(q + (3, -1)) and a coarse field of (1, 0): doubling gives (2, 0), and only the +-1 step reaches the odd
    vector, at cost 0."""
    w, h = 24, 16
    prev = textured(w, h, 3)
    return prev, warp(prev, _uniform(w, h, (3, -1))), _uniform(12, 8, (1, 0)), (10, 8), (3, -1), "NO_PARITY"


def _lone_neighbour(seed, pixel):
    """curr(q) = prev(q + (4, 2)); the coarse field is (0, 0) but for (2, 1) at coarse texel (5, 3)."""
    w, h = 32, 20
    prev = textured(w, h, seed)
    low = _uniform(16, 10, (0, 0))
    low[3, 5] = (2, 1)
    return prev, warp(prev, _uniform(w, h, (4, 2))), low, pixel, (4, 2)


def neighbour_up_left():
    """Pixel (12, 8) lies above coarse texel (6, 4): the right vector is its neighbour (-1, -1), which a 2 x 2 neighbourhood
    of (0 .. 1)^2 does not hold."""
    return _lone_neighbour(4, (12, 8)) + ("NEIGHBOURS_2X2",)


def odd_pixel_rounds_down():
    """Pixel (13, 9) lies above coarse texel (6, 4), whose neighbours reach (5, 3); rounded up it would lie above (7, 5),
    whose neighbours do not."""
    return _lone_neighbour(5, (13, 9)) + ("ROUND_UP",)


def tie_order():
    """All-zero frames: every cost is 0.  Where the coarse field changes from (1, -1) to (-1, 1) both doubled vectors are
    candidates of equal length; the smaller vy wins, (2, -2), and of its +-1 steps the shortest, (1, -1).  With vx before vy
    it would be (-2, 2) and then (-1, 1)."""
    w, h = 16, 8
    low = _uniform(8, 4, (1, -1))
    low[:, 4:] = (-1, 1)
    zeros = np.zeros((h, w, 4), np.uint8)
    return zeros, zeros.copy(), low, (8, 4), (1, -1), "TIE_VX_FIRST"


CASES = {f.__name__: f for f in (saturation, parity, neighbour_up_left, odd_pixel_rounds_down, tie_order)}


def pan_frames(pan, w: int = 200, h: int = 120):
    """Three frames of a synth pan by `pan` per frame: (f0, f1, f2)."""
    from linux_fg_amd import synth
    f0 = synth.make_prev(w, h)
    f1 = synth.translate(f0, pan)
    return f0, f1, synth.translate(f1, pan)


PANS = ((3, -2), (5, 3))
INTERIOR = 24                                   # the pan results hold on pixels at least this far from every edge
