"""The cases that the CPU tests of tests/bicubic_model.py, the host program's test and the GPU tests of
lfg_interpolate_compensated_sampled share, so that they cannot drift apart."""
from __future__ import annotations

import numpy as np

from tests import bicubic_model as bm
from tests import cases, subpel_cases

FACTORS = [0.0, 0.25, 0.3, 0.5, 0.7, 1.0]
# Quarter-pixel vectors at the factors above land on multiples of 1/16 and 1/40 of a pixel only.  23/64 of a vector w / 4 is a
# multiple of 1/256, and w over 256 consecutive values takes every one of them: all 64 phases (and exact in fp32).
PHASE_FACTOR = 23.0 / 64.0
MATCH_SADS = [0, 48, 1020]
# 1 x 1 and 2 x 2: every footprint clamps on all sides; 3 x 5; the wave and workgroup seams (64 x 4 threads); an odd larger one
SIZES = [(1, 1), (2, 2), (3, 5), (64, 4), (65, 5), (130, 9), (97, 61)]
SCENES = ("dense", "full_range", "checkerboard", "step")


def soft_noise(w, h, seed):
    """Bytes in [96, 120): two such frames differ by less than 4 * 24, so the default gate passes some pixels and stops others."""
    return np.random.default_rng(seed).integers(96, 120, (h, w, 4)).astype(np.uint8)


def scene(name, w, h, seed):
    """(prev, curr, mvq int16, mv int8) of one scene: one pair of frames and a field for each route."""
    rng = np.random.default_rng(seed + 1000)
    dense_q = rng.integers(-128, 128, (h, w, 2)).astype(np.int16)          # every residue of 256: every phase at PHASE_FACTOR
    dense_i = rng.integers(-12, 13, (h, w, 2)).astype(np.int8)
    if name == "dense":
        return soft_noise(w, h, seed), soft_noise(w, h, seed + 1), dense_q, dense_i
    if name == "full_range":                                              # holes, the walk, positions outside the image
        prev, curr, mvq = subpel_cases.random_mvq(w, h, seed)
        mv = rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
        mv[rng.random((h, w)) < 0.5] = (2, -1)
        return prev, curr, mvq, mv
    if name == "checkerboard":                                            # the most negative h_r
        return bm.checkerboard(w, h), bm.checkerboard(w, h), dense_q, dense_i
    if name == "step":                                                    # prev overshoots both ways, curr does not: the clamp of p shows
        return bm.step(w, h, 0, 255), np.full((h, w, 4), 100, np.uint8), dense_q, dense_i
    raise KeyError(name)


def all_cases(sizes=SIZES):
    """(id, prev, curr, field) over sizes x scenes x both routes."""
    for k, (w, h) in enumerate(sizes):
        for name in SCENES:
            prev, curr, mvq, mv = scene(name, w, h, 31 * k + len(name))
            yield f"{name}-{w}x{h}-q2", prev, curr, mvq
            yield f"{name}-{w}x{h}-s8", prev, curr, mv


# ---- the shortcut both ways: fields under which the waves of a row (64 pixels each) differ in what they may skip

def shortcut_fields(w=130, h=9):
    """{name: mvq} at t = 0.5, match_sad 1020 (every pixel projects its own vector), on any frames of w x h:
    first_wave_integer  8 quarter pixels (one pixel at t = 0.5) in columns 0..63, 2 beyond: whole waves of either kind;
    one_lane            integer everywhere but one pixel per row;
    horizontal_only / vertical_only  a fraction on one axis alone: the other axis has phase zero wave-wide."""
    def field(wx, wy):
        f = np.zeros((h, w, 2), np.int16)
        f[...] = (wx, wy)
        return f
    first = field(8, 0)
    first[:, 64:] = (2, 0)
    one = field(0, 8)
    one[:, 37] = (0, 6)
    one[:, 101] = (2, 0)
    return {"first_wave_integer": first, "one_lane": one, "horizontal_only": field(6, 8), "vertical_only": field(-8, 2)}


def quality_case():
    """(prev, curr, true mvq, middle) of DESIGN.md section 4.20's scene: the pan of (10, -6) quarter pixels on 8 px cells."""
    prev, curr, middle = subpel_cases.fractional_pan(96, 64, (10, -6), cell=8)
    mvq = np.zeros((64, 96, 2), np.int16)
    mvq[...] = (10, -6)
    return prev, curr, mvq, middle


def squared_error(got, want, border=10):
    d = subpel_cases.interior(got, border).astype(np.int64) - subpel_cases.interior(want, border).astype(np.int64)
    return int((d * d).sum())
