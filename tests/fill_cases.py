"""Cases of the fill plane that the CPU tests (test_fill_model.py) and the GPU tests (test_gpu_fill.py) share: crafted key
images for lfg_hole_fill_plane, and the scenes on which lfg_set_hole_reach(16) must give the walk's bytes."""
from __future__ import annotations

import numpy as np

from tests import bidir_cases as bc, cases, fill_model as fm, mc_model as mc
from tests.c_model import HOLE, key

STATIC = 0
REACHES = (1, 16, 17, 63, 64, 65, 255)
# What the kernels' seams follow from (linux-fg_amd/csrc/hole_fill.hip, lfg_mc.hpp): the row pass gives a lane 4 pixels, so a
# row of 16 lanes ends every 64 pixels and a wave's segment every 256; the column pass gives a workgroup BAND rows.
LANE_ROW_PIXELS, SEGMENT, BAND = 64, 256, 64


def holes(w, h):
    return np.full((h, w), HOLE, np.uint32)


def cross(w, h, at, vector=(5, -3)):
    """All holes but one donor at `at` = (x, y): its arms are the plane."""
    K = holes(w, h)
    K[at[1], at[0]] = key(*vector)
    return K


def cross_at_seams(w, h, reach):
    """The one donor placed so that its right and lower arms end on the first pixel behind a 64-pixel seam and a band seam, where
    such seams exist and the donor fits; the pixel one further, the second behind the seam, is out of reach."""
    def place(size, seam):
        ends = [s for s in range(seam, size, seam) if s - reach >= 0]
        return ends[-1] - reach if ends else size // 2
    return cross(w, h, (place(w, LANE_ROW_PIXELS), place(h, BAND)))


def random_keys(w, h, one_in, seed, static_share=0.25):
    """Donors with probability 1 / one_in, each the key of a random vector in [-127, 127]^2 or, for a quarter of them, the
    static word; everything else a hole."""
    rng = np.random.default_rng(seed)
    vx, vy = rng.integers(-127, 128, (h, w)), rng.integers(-127, 128, (h, w))
    words = (((65535 - (vx * vx + vy * vy)) << 16) | ((vy + 128) << 8) | (vx + 128)).astype(np.uint32)
    words[rng.random((h, w)) < static_share] = STATIC
    return np.where(rng.integers(0, one_in, (h, w)) == 0, words, np.uint32(HOLE)).astype(np.uint32)


def seams(w, h, reach, seed=11):
    """For every 64-pixel seam s of a row (the ends of a 16-lane row and, every fourth, of a segment) donors at s - reach and
    s - 1 + reach, and for every band seam of a column the same, each on a line of its own where the image has that many: from
    s - reach the first pixel behind the seam is at distance reach and the second at reach + 1, from s - 1 + reach the last pixel
    before the seam and the one before it.  Random vectors, so that a donor wrongly kept or dropped changes a minimum."""
    rng = np.random.default_rng(seed)
    K = holes(w, h)
    line = 0
    for s in range(LANE_ROW_PIXELS, w, LANE_ROW_PIXELS):
        for x in (s - reach, s - 1 + reach):
            if 0 <= x < w:
                K[(7 * line + 3) % h, x] = key(int(rng.integers(-127, 128)), int(rng.integers(-127, 128)))
                line += 1
    for s in range(BAND, h, BAND):
        for y in (s - reach, s - 1 + reach):
            if 0 <= y < h:
                K[y, (7 * line + 3) % w] = key(int(rng.integers(-127, 128)), int(rng.integers(-127, 128)))
                line += 1
    return K


def patterns(w, h, reach):
    """(name, K) of the crafted key images of one size and reach."""
    yield "cross", cross_at_seams(w, h, reach)
    yield "seams", seams(w, h, reach)
    for one_in in (2, 50, 2000):
        yield f"1/{one_in}", random_keys(w, h, one_in, seed=one_in + w)


# ---- scenes for lfg_set_hole_reach through the three calls

def scene_fields(scene):
    """((prev, truth, curr), fwd, bwd): fill_model.fast_scene with its true field both ways: bwd is +pan on prev's grid and +shift
    on the square's place in prev."""
    (prev, truth, curr), fwd = fm.fast_scene(**scene)
    bwd = np.zeros_like(fwd)
    bwd[...] = scene["pan"]
    (x, y), sq = scene["at"], scene["sq"]
    bwd[y:y + sq, x:x + sq] = scene["shift"]
    return (prev, truth, curr), fwd, bwd


def moving_square_fields():
    """(prev, curr, fwd, bwd): mc_model.moving_square with its true field both ways."""
    prev, curr, (x, y) = mc.moving_square()
    fwd, bwd = np.zeros(prev.shape[:2] + (2,), np.int8), np.zeros(prev.shape[:2] + (2,), np.int8)
    fwd[y:y + 16, x + 12:x + 28] = (-12, 0)
    bwd[y:y + 16, x:x + 16] = (12, 0)
    return prev, curr, fwd, bwd


def equivalence_cases():
    """(name, prev, curr, fwd, bwd, mask, match_sad, tolerance) on which reach 16 must give the walk's bytes: the walk-reach cases
    of tests/cases.py (with its blank field, and with the static run as the mask), the moving square and scene B.  mask is None
    where the case has none: the masked call then runs under lfg_static_mask's model at tolerance 0."""
    prev, curr, fwd, bwd, blank = bc.walk_reach()
    yield "walk_reach", prev, curr, fwd, bwd, cases.walk_reach_static_run(), cases.WALK_REACH_MATCH_SAD, 0
    yield "walk_reach_blank", prev, curr, blank, blank, np.zeros((40, 40), np.uint8), cases.WALK_REACH_MATCH_SAD, 0
    yield ("moving_square", *moving_square_fields(), None, 48, 1)
    (prev, _, curr), fwd, bwd = scene_fields(fm.SCENE_B)
    yield "scene_b", prev, curr, fwd, bwd, None, 48, 1
