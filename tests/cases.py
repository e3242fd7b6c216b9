"""Inputs that the CPU tests of the models and the GPU tests share, so that the two cannot drift apart: the factors of the
compensated interpolator, the scene on which lfg_interpolate samples (tests/test_sampling_scene.py,
tests/test_gpu_interpolate_scale.py), the scene and the CPU chain of the dispatch tests (tests/test_gpu_dispatch.py), and the hand-made
cases of test_refine_model.py, test_mc_model.py and test_pyramid_model.py that are stated through the public inputs alone."""
from __future__ import annotations

import itertools

import numpy as np

from tests import mc_model as mc
from tests import pyramid_model as pm
from tests import refine_model as rm

# ---- factors of lfg_interpolate_compensated
#
# At a dyadic factor every product v * s, u * t of a whole-pixel vector is exact in fp32, so any rewrite of the position
# arithmetic that is exact in real numbers gives the same bytes.  The inexact ones are those that tell the mutants of
# tests/mc_model.c from the model (test_mc_model.py: test_inexact_factors_tell_the_mutants_from_the_model): all four tell the
# first two, 0.9 and 5/6 the third; 1/3, 2/3, 0.2, 0.4 and 0.6 told none on the same input, 1/10 and 1/6 only the first.  The
# last two approach the header's limits ("t = 1 gives
# curr", t = 0) without reaching them.
DYADIC_FACTORS = [0.0, 0.25, 0.5, 0.75, 1.0]
INEXACT_FACTORS = [0.3, 0.7, 0.9, 5.0 / 6.0]
LIMIT_FACTORS = [float(np.nextafter(np.float32(1.0), np.float32(0.0))), float(np.finfo(np.float32).tiny)]


def textured(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def field(kind, w, h, seed):
    """(prev, curr, mv int8) for the vector fields that need no estimator: "uniform", "piecewise" or dense "random"."""
    from linux_fg_amd import synth
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    mv = np.zeros((h, w, 2), np.int8)
    if kind == "uniform":
        mv[...] = rng.integers(-20, 21, 2)
        curr = synth.translate(prev, tuple(-int(v) for v in mv[0, 0]), synth.BASE_SEED + seed)
    elif kind == "piecewise":             # four quadrants with their own vectors: collisions along the seams
        vs = rng.integers(-12, 13, (4, 2))
        mv[: h // 2, : w // 2], mv[: h // 2, w // 2:], mv[h // 2:, : w // 2], mv[h // 2:, w // 2:] = vs
        curr = np.clip(prev.astype(np.int16) + rng.integers(-6, 7, prev.shape), 0, 255).astype(np.uint8)
    else:                                 # dense random over the full byte range: holes and conflicts everywhere
        assert kind == "random", kind
        mv = rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
        curr = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return prev, curr, mv


def sampling_scene(w, h, seed):
    """(prev, curr, mv int8) on which lfg_interpolate samples, under both semantics: prev and curr are independent uniform
    noise and the vectors are drawn per pixel, so that every row and column carries non-trivial ones -- about 55 % are (0, 0)
    (both samples inside the image under either semantics), 35 % small, from [-3, 3]^2 (under the reference semantics a
    sample of theirs leaves [0, 1] and reads as 0; under the intended semantics both move by a few pixels, mostly to
    fractional positions), 10 % from the full byte range.  What the scene is held to: tests/test_sampling_scene.py."""
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    curr = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    small = rng.integers(-3, 4, (h, w, 2)).astype(np.int8)
    large = rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
    r = rng.random((h, w))
    mv = np.zeros((h, w, 2), np.int8)
    mv[r < 0.45] = small[r < 0.45]
    mv[r < 0.10] = large[r < 0.10]
    return prev, curr, mv


SAMPLING_FACTORS = (0.5, 0.3)                       # a dyadic factor and one that is inexact in fp32


def sampling_scene_of(w, h):
    """The sampling scene the CPU test of its power and the GPU tests of lfg_interpolate_scale both take at w x h."""
    return sampling_scene(w, h, 1000 * w + h)


def warp(prev, field):
    """curr(q) = prev(q + v(q)), 0 where q + v(q) leaves the image (the cost's own convention for prev outside)."""
    h, w = prev.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs + field[..., 0].astype(int), ys + field[..., 1].astype(int)
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    curr = np.zeros_like(prev)
    curr[inside] = prev[sy[inside], sx[inside]]
    return curr


# ---- the dispatch of lfg_interpolate_frames[_multi]: settings, scene and CPU chain
#
# A setting is (estimator, radius, interpolator, semantics): "full" / "pyramid", -1 .. 2, "shader" / "compensated", 0 / 1
# (LFG_SEMANTICS_REFERENCE / _INTENDED).  The fused-motion flag is no part of it: the header defines the same bytes with and
# without it on every branch.

ESTIMATORS = ("full", "pyramid")
RADII = (-1, 0, 1, 2)
INTERPOLATORS = ("shader", "compensated")
SEMANTICS = (0, 1)
SETTINGS = list(itertools.product(ESTIMATORS, RADII, INTERPOLATORS, SEMANTICS))
MATRIX_FACTOR = 0.3                                 # the single call of the matrix
MATRIX_FACTORS = [0.25, 5.0 / 6.0, 0.5, 0.9]        # its multi call


def matrix_scene(w: int = 200, h: int = 120):
    """(prev, curr) that tells the settings apart (test_mc_model.py: test_matrix_scene_tells_the_settings_apart): a panned
    background, two squares with motions of their own -- moving edges for the refinement radii, vectors of 2 px and more for
    the two semantics of the shader's interpolation -- and a flat patch, where the full search's two tie orders differ."""
    prev, curr = rm.moving_objects(w, h, pan=(4, -2), squares=((24, (60, 40), (10, 6)), (32, (120, 56), (-14, 4))))[:2]
    for f in (prev, curr):
        f[76:108, 8:48] = (90, 140, 200, 255)
    return prev, curr


def small_scene(w: int, h: int, seed: int):
    """A pair of any size, 1 x 1 included: a pan, a moving square where it fits, and a flat patch.  For the tests of the
    temporaries: below 16 px it is a bare pan and does not tell every setting apart -- which branch runs is the matrix's
    business (matrix_scene), what the temporaries hold after a change of size is this one's."""
    from linux_fg_amd import synth
    prev = synth.make_prev(w, h, synth.BASE_SEED + seed)
    curr = synth.translate(prev, (3, -2), synth.BASE_SEED + seed)
    s = min(w, h) // 4
    if s >= 4:
        tex = textured(s, s, seed)
        prev[s:2 * s, s:2 * s] = tex
        curr[s + 2:2 * s + 2, s + 6:2 * s + 6] = tex
        prev[h - s:, :s] = curr[h - s:, :s] = (10, 200, 30, 255)
    return prev, curr


class Chain:
    """The CPU chain on one pair: the estimator's model, then the refine model when radius >= 0, then the interpolation
    model.  Vectors and frames are kept, so each is computed once per (estimator, semantics, radius, interpolator, factor,
    match_sad) however many tests ask; the frames returned are shared: compare, do not write."""

    def __init__(self, prev, curr):
        self.prev, self.curr = prev, curr
        self._estimated, self._refined, self._frames = {}, {}, {}

    def vectors(self, estimator, radius, semantics):
        """The vectors the interpolator of a setting is given."""
        k = (estimator, semantics if estimator == "full" else None)      # the pyramid does not depend on the semantics
        if k not in self._estimated:
            if estimator == "pyramid":
                self._estimated[k] = pm.motion_pyramid(self.prev, self.curr, 2, 16, 2)
            else:
                import oracle
                self._estimated[k] = oracle.motion(self.prev, self.curr, semantics=semantics).astype(np.int8)
        if radius < 0:
            return self._estimated[k]
        if k + (radius,) not in self._refined:
            self._refined[k + (radius,)] = rm.refine(self.prev, self.curr, self._estimated[k], radius)
        return self._refined[k + (radius,)]

    def frames(self, setting, factors, match_sad=mc.DEFAULT_MATCH_SAD):
        """The frames that lfg_interpolate_frames[_multi] must give under `setting`, one per factor."""
        estimator, radius, interpolator, semantics = setting
        out = []
        for t in factors:
            k = (tuple(setting), float(t), match_sad if interpolator == "compensated" else None)
            if k not in self._frames:
                mv = self.vectors(estimator, radius, semantics)
                if interpolator == "compensated":
                    self._frames[k] = mc.interpolate_compensated(self.prev, self.curr, mv, t, match_sad)
                else:
                    import oracle
                    self._frames[k] = oracle.interpolate(self.prev, self.curr, mv.astype(np.float32), t, semantics=semantics)
            out.append(self._frames[k])
        return out


def same_by_definition(a, b) -> bool:
    """Two settings that the header defines to give the same bytes on any input: the pyramid's vectors, the refinement and
    the compensated interpolation depend on neither semantics."""
    return a[:3] == b[:3] and a[0] == "pyramid" and a[2] == "compensated"


# ---- lfg_motion_refine: the hand-made cases of test_refine_model.py

def refine_straight_edge(radius: int, vertical: bool):
    """(prev, curr, mv, truth): two regions with their own vectors, split by a straight line; mv has the block matcher's
    error, a 3 px band past the edge holding the other side's vector.  Every pixel comes out with its own region's."""
    w, h, e = 48, 40, 21
    va, vb = np.array([3, -2], np.int8), np.array([-5, 1], np.int8)
    ys, xs = np.mgrid[0:h, 0:w]
    pos = xs if vertical else ys
    truth = np.where((pos < e)[..., None], va, vb).astype(np.int8)
    mv = np.where((pos < e + 3)[..., None], va, vb).astype(np.int8)
    prev = textured(w, h, 20 + radius)
    return prev, warp(prev, truth), mv, truth


def refine_tie_case(vectors_):
    """17 x 17 zero frames (every cost 0); pixel (8, 8)'s candidates set to `vectors_` in offset order, the rest (7, 7)."""
    mv = np.zeros((17, 17, 2), np.int8)
    mv[...] = (7, 7)
    for (dx, dy), v in zip(rm.OFFSETS, vectors_):
        mv[8 + dy, 8 + dx] = v
    z = np.zeros((17, 17, 4), np.uint8)
    return z, z, mv


REFINE_TIES = [                                     # (candidates of pixel (8, 8), the one that wins)
    ([(5, 5), (3, 0), (-3, 0), (0, 3), (0, -3)], (0, -3)),            # |v|^2 = 9 each: smallest vy
    ([(5, 5), (3, 0), (-3, 0), (0, 3)], (-3, 0)),                     # (3,0) / (-3,0): same vy, smallest vx
    ([(5, 5), (0, -3), (1, 2), (-2, -1)], (-2, -1)),                  # |v|^2 = 5 beats 9; (-2,-1) has the smaller vy
    ([(5, 5), (4, 4), (0, 0)], (0, 0)),
    ([(-9, 0), (9, 0)], (-9, 0)),
]


def refine_cost_before_length():
    """(prev, curr, mv): curr is prev moved by (6, 2) and the field is (0, 0) but for one (6, 2) at (16, 8)."""
    w, h = 24, 16
    prev = textured(w, h, 30)
    curr = warp(prev, np.broadcast_to(np.array([6, 2], np.int8), (h, w, 2)))
    mv = np.zeros((h, w, 2), np.int8)
    mv[8, 16] = (6, 2)                             # a candidate of (12, 8) (offset (4, 0)) and of (8, 8) (offset (8, 0))
    return prev, curr, mv


def refine_candidates_outside():
    """A 4 x 1 frame: pixel 0's only candidate is its own (x = 4 and x = 8 are outside), even though (0, 0) would fit
    better; an outside position read as (0, 0) would win here."""
    prev = textured(4, 1, 40)
    mv = np.array([[(2, 0), (0, 0), (0, 0), (0, 0)]], np.int8)
    return prev, prev.copy(), mv                   # (0, 0) costs 0


def refine_prev_outside_zero():
    """curr is 0 and prev 255: a vector that moves the whole window out of the image costs 0 and beats (0, 0), which costs
    255 per channel.  With prev clamped to the edge both would cost the same and (0, 0) would win on length."""
    w, h = 12, 12
    prev = np.full((h, w, 4), 255, np.uint8)
    curr = np.zeros((h, w, 4), np.uint8)
    mv = np.zeros((h, w, 2), np.int8)
    mv[6, 6] = (100, 0)
    return prev, curr, mv


# ---- lfg_interpolate_compensated: the hand-made 8 x 8 cases of test_mc_model.py.  At t = 0.5 a vector v projects by
# floor(v * 0.5 + 0.5), i.e. v / 2 for even v.

def mc_zeros(textured_frames: bool = False):
    """8 x 8 frames and zero vectors.  Flat black: every pixel matches, even at match_sad 0, but every generated frame is
    black too.  Textured (for match_sad 1020, where every pixel matches as well): the same projection, and a generated frame
    that shows which vector each pixel was sampled with."""
    if textured_frames:
        return textured(8, 8, 61), textured(8, 8, 62), np.zeros((8, 8, 2), np.int8)
    return np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 2), np.int8)


def mc_collision(textured_frames: bool = False):
    """(prev, curr, mv, {(x, y): the vector whose key wins there})"""
    prev, curr, mv = mc_zeros(textured_frames)
    mv[4, 5] = (-2, 0)          # -> (4, 4), |v|^2 = 4
    mv[4, 6] = (-4, 0)          # -> (4, 4), |v|^2 = 16: wins (and over (4,4)'s own (0,0))
    mv[2, 4] = (0, 2)           # -> (4, 3)
    mv[4, 4] = (0, -2)          # -> (4, 3): the same |v|^2, the smaller vy wins
    mv[6, 2] = (2, 0)           # -> (3, 6)
    mv[6, 4] = (-2, 0)          # -> (3, 6): the same |v|^2 and vy, the smaller vx wins
    return prev, curr, mv, {(4, 4): (-4, 0), (4, 3): (0, -2), (3, 6): (-2, 0)}


def mc_unmatched_source():
    """(prev, curr, mv): (3, 3) projects to (4, 3) at match_sad 200 and not at 199."""
    prev, curr, mv = mc_zeros()
    curr[3, 3] = (200, 0, 0, 0)                          # against prev(5, 3) = 0: SAD 200
    mv[3, 3] = (2, 0)                                    # -> (4, 3)
    return prev, curr, mv


def mc_projection_outside(textured_frames: bool = False):
    prev, curr, mv = mc_zeros(textured_frames)
    mv[0, 0] = (0, -2)                                   # -> (0, -1)
    mv[7, 7] = (4, 0)                                    # -> (9, 7)
    return prev, curr, mv


def mc_revealed_and_covered():
    """(prev, curr, mv, obj): an object moves from (4, 2) to (6, 2) over black, v(6, 2) = (-2, 0); match_sad 0."""
    prev, curr, mv = mc_zeros()
    obj = (200, 100, 50, 255)
    prev[2, 4] = obj
    curr[2, 6] = obj
    mv[2, 6] = (-2, 0)
    return prev, curr, mv, obj


def mc_row_projected_to_the_top():
    """(prev, curr, mv): textured 8 x 8, row 3 moves up by 4 and lands on row 1, whose prev sample (y = -0.5) is outside:
    at t = 0.5 and match_sad 1020 row 1 of the output is curr's row 3."""
    prev, curr = textured(8, 8, 41), textured(8, 8, 42)
    mv = np.zeros((8, 8, 2), np.int8)
    mv[3, :] = (0, -4)
    return prev, curr, mv


# ---- the hole walk's reach through the public calls (the compensated, the masked and, with tests/bidir_cases.py, the
# bidirectional one).  40 x 40, independent random frames, match_sad 1020 (every pixel matches), every vector (127, 0): at
# t = 0.5 and 0.3 it projects 64 and 89 columns to the right, out of the image, so K is all holes -- but for mv(19, 20) =
# (2, 0), which lands on (20, 20) at both factors: floor(2 * 0.5 + 0.5) = floor(2 * 0.7 + 0.5) = 1.  Only holes that find
# (20, 20) within the walk's 16 steps are filled with (2, 0) and not (0, 0): row 20 and column 20 at 4 .. 36, both included.

WALK_REACH_FACTORS = (0.5, 0.3)
WALK_REACH_MATCH_SAD = 1020
WALK_REACH_TIPS = ((4, 20), (36, 20), (20, 4), (20, 36))           # (x, y) at distance 16: filled
WALK_REACH_PAST = ((3, 20), (37, 20), (20, 3), (20, 37))           # at 17: not


def mc_walk_reach():
    """(prev, curr, mv, blank): the case above, and `blank`, the field with (127, 0) everywhere, whose K is all holes."""
    rng = np.random.default_rng(7)
    prev = rng.integers(0, 256, (40, 40, 4), dtype=np.uint8)
    curr = rng.integers(0, 256, (40, 40, 4), dtype=np.uint8)
    blank = np.zeros((40, 40, 2), np.int8)
    blank[...] = (127, 0)
    mv = blank.copy()
    mv[20, 19] = (2, 0)
    return prev, curr, mv, blank


def walk_reach_plus():
    """The 65 pixels of the 40 x 40 image that see (20, 20) within 16 steps along an axis, (20, 20) included, as a mask."""
    plus = np.zeros((40, 40), bool)
    plus[20, 4:37] = plus[4:37, 20] = True
    return plus


def walk_reach_static_run():
    """The mask of the masked call's second run: (26 .. 29, 20) static, between (20, 20) and the tip (36, 20)."""
    mask = np.zeros((40, 40), np.uint8)
    mask[20, 26:30] = 255
    return mask


def check_walk_reach(frame, blank_frame, what, static_run=False):
    """`frame` (of mv) differs from `blank_frame` (of blank) on the plus and nowhere else: the tips at distance 16 do, the
    pixels one step further do not.  static_run: both frames are the masked call's under walk_reach_static_run() -- its four
    pixels are the static mix in both, and the walk passes over them, so the plus loses them and nothing else: (36, 20) still
    differs."""
    differs = (frame != blank_frame).any(axis=-1)
    want = walk_reach_plus()
    if static_run:
        want[20, 26:30] = False
    assert differs.sum() == (61 if static_run else 65), (what, int(differs.sum()))
    assert (differs == want).all(), (what, np.argwhere(differs != want)[:4].tolist())
    assert all(differs[y, x] for x, y in WALK_REACH_TIPS), what
    assert not any(differs[y, x] for x, y in WALK_REACH_PAST), what


# ---- lfg_motion_pyramid: the tie of test_pyramid_model.py

def pyramid_tie(axis: int):
    """(prev, curr, params, the vector of the interior): curr repeats every 4 px along one axis and prev is curr moved by 2
    along it: v and -v match exactly.  Of the two the smaller vy (vertical) or, vy equal, the smaller vx (horizontal) wins."""
    rng = np.random.default_rng(5)
    H, W = 48, 64
    if axis == 0:
        row = rng.integers(0, 256, (H, 4, 4), dtype=np.uint8)
        curr = np.tile(row, (1, W // 4, 1))
    else:
        col = rng.integers(0, 256, (4, W, 4), dtype=np.uint8)
        curr = np.tile(col, (H // 4, 1, 1))
    prev = np.roll(curr, 2, axis=1 - axis)
    return prev, curr, (1, 4, 2), ((-2, 0) if axis == 0 else (0, -2))
