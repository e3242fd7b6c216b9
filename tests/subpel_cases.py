"""Scenes and hand-worked cases that the CPU tests of tests/subpel_model.py and the GPU tests of lfg_motion_subpel and
lfg_interpolate_compensated_subpel share, so that the two cannot drift apart."""
from __future__ import annotations

import numpy as np

from tests import cases

PANS = [(10, -6), (6, 2), (-5, 3), (7, 9)]           # quarter pixels per frame; the first two are even: a middle frame exists
FACTORS = [0.0, 0.25, 0.5, 0.7, 1.0]
MATCH_SADS = [0, 48, 1020]


def rounded(wq):
    """The integer vector nearest to the quarter-pixel vector wq, halves rounded up: what an integer estimator is asked for."""
    return tuple(int(np.floor(c / 4 + 0.5)) for c in wq)


def _master_frames(w, h, offsets, cell, seed):
    """The rounded 4 x 4 box means of one random master (bytes on cell x cell cells, 4 x the size plus a margin of 40 frame
    pixels on every side) at the quarter-pixel `offsets`."""
    pad = 40
    rng = np.random.default_rng(seed)
    mh, mw = (h + 2 * pad) * 4, (w + 2 * pad) * 4
    coarse = rng.integers(0, 256, (mh // cell + 2, mw // cell + 2, 4)).astype(np.int64)
    master = np.kron(coarse, np.ones((cell, cell, 1), np.int64))[:mh, :mw]
    out = []
    for ox, oy in offsets:
        assert max(abs(ox), abs(oy)) <= pad * 4, (ox, oy)
        y0, x0 = pad * 4 + oy, pad * 4 + ox
        sub = master[y0:y0 + h * 4, x0:x0 + w * 4].reshape(h, 4, w, 4, 4).sum(axis=(1, 3))
        out.append(((sub + 8) >> 4).astype(np.uint8))     # the mean of 16, halves rounded up
    return out


def fractional_pan(w, h, wq, cell=8, seed=7):
    """(prev, curr, middle or None): a master of random bytes on cell x cell cells at 4 x the size plus a margin; a frame is
    the rounded 4 x 4 box mean of the master at a quarter-pixel offset, prev at (0, 0), curr at wq, so curr(q) ~ prev(q + wq / 4),
    and for even wq the frame at wq / 2 is the true middle frame.  prev sits on the cell grid: with cell = 8 its pixels never
    straddle a cell, and curr is prev's bilinear sample at wq up to the rounding of the means -- the sharpest content there is,
    and an exact one for this one pair.  (A later pair of the same pan, pan_stream's, has no such anchor: 2 px cells are
    aliasing there, which no vector explains.  Streams that are judged for quality take wider cells.)"""
    even = wq[0] % 2 == 0 and wq[1] % 2 == 0
    frames = _master_frames(w, h, [(0, 0), tuple(wq)] + ([(wq[0] // 2, wq[1] // 2)] if even else []), cell, seed)
    return frames[0], frames[1], frames[2] if even else None


def pan_stream(w, h, wq, n, cell=8, seed=7):
    """n frames of the same pan: frame k is the master at k * wq."""
    return _master_frames(w, h, [(k * wq[0], k * wq[1]) for k in range(n)], cell, seed)


def pan_vectors(w, h, wq):
    mv = np.zeros((h, w, 2), np.int8)
    mv[...] = rounded(wq)
    return mv


def interior(a, border=10):
    return a[border:-border, border:-border]


# ---- known answers of lfg_motion_subpel: (prev, curr, mv, radius, {(x, y): (wx, wy)}); every other pixel is only held to the model

def flat(seed=3):
    """Zero frames -- a texel outside the image reads as 0 too, so every window is flat wherever the vector points -- and random
    vectors over the full byte range with +-127 and -128 among them: the output is 4 v, v = -128 read as -127; at +-127 the
    candidates beyond +-508 drop."""
    w, h = 24, 16
    mv = np.random.default_rng(seed).integers(-128, 128, (h, w, 2)).astype(np.int8)
    mv[0, 0], mv[0, 1], mv[1, 0], mv[1, 1] = (127, 127), (-127, 127), (-128, -128), (127, -128)
    z = np.zeros((h, w, 4), np.uint8)
    want = {(x, y): tuple(4 * max(int(c), -127) for c in mv[y, x]) for y in range(h) for x in range(w)}
    return z, z.copy(), mv, 1, want


def step_edge(quarters):
    """A vertical step 0 | 160 between columns 7 and 8, and curr = prev moved by quarters / 4 px (-3 .. 3, not 0), radius 0,
    vectors 0.  For quarters > 0 column 7 of curr is 40 * quarters, which among the candidates only dx = quarters gives
    (prevq(7, (d, 0)) = 40 d for d >= 0, 0 below); for quarters < 0 column 8 is 160 + 40 * quarters and prevq(8, (d, 0)) =
    160 + 40 d for d <= 0.  Stage 1 ends on the nearest even step (on 0 in a tie, where the integer wins), stage 2 on
    `quarters`; dy ties at every step and stays 0.  Flat windows elsewhere give (0, 0)."""
    assert quarters != 0 and abs(quarters) <= 3
    w, h = 16, 6
    prev = np.zeros((h, w, 4), np.uint8)
    prev[:, 8:] = 160
    curr = prev.copy()
    x = 7 if quarters > 0 else 8
    curr[:, x] = 40 * quarters if quarters > 0 else 160 + 40 * quarters
    want = {(c, r): (0, 0) for r in range(1, h - 1) for c in range(w)}      # (rows 0 and h - 1 see the outside, which is no step edge)
    for r in range(1, h - 1):
        want[(x, r)] = (quarters, 0)
    return prev, curr, np.zeros((h, w, 2), np.int8), 0, want


def off_image():
    """prev is 255, curr 0, and v = (5, 0) at (6, 6) of a 12 x 12 frame points at the last column.  Outside reads as 0, so each
    quarter further right costs less: 1020, 512 at +2, 256 at +3 -- the answer is 4 v + (3, 0).  With prev clamped to the edge
    every candidate would cost 1020 and the integer would win."""
    w = h = 12
    prev = np.full((h, w, 4), 255, np.uint8)
    curr = np.zeros((h, w, 4), np.uint8)
    mv = np.zeros((h, w, 2), np.int8)
    mv[6, 6] = (5, 0)
    return prev, curr, mv, 0, {(6, 6): (23, 0)}


def fraction_tie(horizontal_only: bool):
    """Radius 0 at q = (5, 5) with v = (3, 2): prev(q + v) is 0 and its left and right neighbours are 160 -- and, unless
    horizontal_only, those above and below too -- and curr(q) is 80.  Half a pixel towards any bright neighbour costs 0, the
    integer 320: the four (two) half steps tie, and so do diagonal steps of greater length.  The smallest (|d|^2, dy, dx) is
    d = (0, -2), decided by dy; with horizontal_only d = (-2, 0), decided by dx.  Stage 2 finds nothing better around it.
    (v is not 0 so that the shortest w is another candidate than the smallest d.)"""
    w = h = 14
    prev = np.zeros((h, w, 4), np.uint8)
    curr = np.zeros((h, w, 4), np.uint8)
    mv = np.zeros((h, w, 2), np.int8)
    mv[5, 5] = (3, 2)
    prev[7, 7] = prev[7, 9] = 160                     # q + v = (8, 7)
    if not horizontal_only:
        prev[6, 8] = prev[8, 8] = 160
    curr[5, 5] = 80
    return prev, curr, mv, 0, {(5, 5): (10, 8) if horizontal_only else (12, 6)}


def rounding():
    """Columns 0 | 2 and curr = 1 at column 7, radius 0: a quarter step gives (1 * 4 * 2 + 8) >> 4 = 1 and costs 0, as the half
    step does ((2 * 4 * 2 + 8) >> 4 = 1): stage 1 ends on (2, 0), stage 2 on the shorter (1, 0).  Rounding with + 7 makes the
    quarter step 0."""
    w, h = 16, 6
    prev = np.zeros((h, w, 4), np.uint8)
    prev[:, 8:] = 2
    curr = prev.copy()
    curr[:, 7] = 1
    return prev, curr, np.zeros((h, w, 2), np.int8), 0, {(7, r): (1, 0) for r in range(1, h - 1)}


KNOWN = {
    "flat": flat,
    **{f"step_edge_{k}": (lambda k=k: step_edge(k)) for k in (-3, -2, -1, 1, 2, 3)},
    "off_image": off_image,
    "fraction_tie_dy": lambda: fraction_tie(False),
    "fraction_tie_dx": lambda: fraction_tie(True),
    "rounding": rounding,
}


def random_vectors(w, h, seed):
    """(prev, curr, mv): curr is prev with noise, so costs are finite and differ, and the vectors cover the full byte range with
    +-127 and -128 among them."""
    rng = np.random.default_rng(seed)
    prev = cases.textured(w, h, seed)
    curr = np.clip(prev.astype(np.int16) + rng.integers(-40, 41, prev.shape), 0, 255).astype(np.uint8)
    mv = rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
    mv.reshape(-1)[:2] = (-128, 127)
    if mv.size >= 8:
        mv.reshape(-1)[-2:] = (127, -127)
    small = rng.random((h, w)) < 0.5                  # half of them short, so that most windows lie inside the image
    mv[small] = rng.integers(-4, 5, (h, w, 2)).astype(np.int8)[small]
    return prev, curr, mv


# ---- lfg_interpolate_compensated_subpel

def random_mvq(w, h, seed):
    """(prev, curr, mvq int16): independent noise frames and vectors of which a third cover the full int16 range (the clamp),
    a third the clamped range and a third a few pixels, fractions included."""
    rng = np.random.default_rng(seed)
    prev, curr = cases.textured(w, h, seed), cases.textured(w, h, seed + 500)
    r = rng.random((h, w))
    mvq = rng.integers(-32768, 32768, (h, w, 2)).astype(np.int16)
    mid = rng.integers(-520, 521, (h, w, 2)).astype(np.int16)
    near = rng.integers(-24, 25, (h, w, 2)).astype(np.int16)
    mvq[r < 2 / 3] = mid[r < 2 / 3]
    mvq[r < 1 / 3] = near[r < 1 / 3]
    mvq.reshape(-1)[:2] = (-32768, 32767)
    return prev, curr, mvq


COLLISION_FACTOR = 0.4


def collision():
    """(prev, curr, mvq, (x, y), winner): zero 8 x 8 frames, every pixel matches.  At t = 0.4 (s = 0.6) the source (6, 4) with
    w = (-9, 0) moves by floor(-2.25 * 0.6 + 0.5) = -1 and the source (7, 4) with w = (-11, 0) by floor(-2.75 * 0.6 + 0.5) = -2:
    both land on (5, 4), next to that pixel's own (0, 0).  Both vectors have the integer part -3; the longer one wins, which
    only an order on the quarter-pixel components can tell."""
    z = np.zeros((8, 8, 4), np.uint8)
    mvq = np.zeros((8, 8, 2), np.int16)
    mvq[4, 6] = (-9, 0)
    mvq[4, 7] = (-11, 0)
    return z, z.copy(), mvq, (5, 4), (-11, 0)


def revealed_and_covered():
    """cases.mc_revealed_and_covered in quarter pixels: (prev, curr, mvq, obj), match_sad 0."""
    prev, curr, mv, obj = cases.mc_revealed_and_covered()
    return prev, curr, (4 * mv.astype(np.int16)), obj


def anchor_inputs():
    """(name, prev, curr, mv int8 with components in [-127, 127]) on which the route with 4 mv must equal the integer one."""
    out = []
    for i, (w, h) in enumerate([(1, 1), (17, 9), (65, 5), (97, 61)]):
        prev, curr = cases.small_scene(w, h, 70 + i)
        mv = np.random.default_rng(i).integers(-127, 128, (h, w, 2)).astype(np.int8)
        out.append((f"small_scene_{w}x{h}", prev, curr, mv))
        mv = mv.copy()
        mv[np.random.default_rng(i + 9).random((h, w)) < 0.7] = (3, -2)      # mostly the scene's own pan
        out.append((f"small_scene_pan_{w}x{h}", prev, curr, mv))
    for name, make in (("collision", cases.mc_collision), ("unmatched", cases.mc_unmatched_source),
                       ("outside", cases.mc_projection_outside), ("revealed", cases.mc_revealed_and_covered),
                       ("row_to_top", cases.mc_row_projected_to_the_top), ("walk_reach", cases.mc_walk_reach)):
        prev, curr, mv = make()[:3]
        out.append((name, prev, curr, mv))
    prev, curr, mv = cases.field("random", 70, 50, 57)
    out.append(("random", prev, curr, np.maximum(mv, -127).astype(np.int8)))
    return out
