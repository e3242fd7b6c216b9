"""CPU model of lfg_frame_ssim and lfg_frame_ssim_summarize, restated in numpy and Python integers from include/linuxfg_hip.h
(not from csrc/frame_ssim.hip), its mutants, and the scenes that the CPU and GPU tests of the measure share.

``frame_ssim(a, b, mask)`` is the record (windows, sum tuple of 4, hist tuple of 65, worst) as lfg_frame_ssim writes it --
``record(quotients(a, b), mask)``, for a caller that wants several masks of one pair --, ``add(r, s)`` what accumulate = 1 makes of two records, ``summarize(record, mask)`` the dict of lfg_frame_ssim_summarize's
figures, or None where the call returns LFG_ERR_INVALID.  The quotient floor(|N| 2^24 / D) needs 82 bits, so it is taken in
Python integers; everything before it fits numpy's int64.

A mutant is the model with one rule bent, to show that the tests' scenes can tell (tests/test_ssim_model.py):
    narrow_n, narrow_d   the product N, or D, keeps its low 32 bits only (N signed, D unsigned and at least 1).  The header's
                         vars and covar themselves never leave 32 bits (vars <= 133,171,200, |covar| <= 66,585,600), so a
                         32-bit vars or covar IS the model; what needs 64 bits is each one's product, and that is what is bent;
    round                the quotient rounded to nearest instead of truncated toward zero;
    stride8              windows at every second block position;
    remainder            the multiple of 4 is measured from the right and bottom edge, so the remainder is looked at;
    hist_all             m over all four channels whatever the mask;
    windows_not_added    add() keeps the first record's window count;
    worst_rightmost      a tie of `worst` goes to the rightmost window of the topmost row."""
from __future__ import annotations

import math

import numpy as np

from tests import cases
from tests import diff_model as dm

ONE = 1 << 24
MASKS = (0xF, 0x7, 0x8, 0x5)
NO_WINDOW = (1 << 64) - 1
MUTANTS = ("narrow_n", "narrow_d", "round", "stride8", "remainder", "hist_all", "windows_not_added", "worst_rightmost")


def window_sums(a: np.ndarray, b: np.ndarray, mutant=None):
    """(s1, s2, ss, s12), each (bh - 1, bw - 1, 4) int64: the sums over the 8 x 8 window at every block position."""
    assert a.shape == b.shape and a.shape[2] == 4 and a.dtype == b.dtype == np.uint8 and a.shape[0] >= 8 and a.shape[1] >= 8
    h, w = (a.shape[0] >> 2) << 2, (a.shape[1] >> 2) << 2
    y0, x0 = (a.shape[0] - h, a.shape[1] - w) if mutant == "remainder" else (0, 0)
    x, y = a[y0:y0 + h, x0:x0 + w].astype(np.int64), b[y0:y0 + h, x0:x0 + w].astype(np.int64)
    step = 8 if mutant == "stride8" else 4

    def boxes(v):
        c = np.zeros((h + 1, w + 1, 4), np.int64)
        c[1:, 1:] = v.cumsum(0).cumsum(1)
        return (c[8:, 8:] - c[:-8, 8:] - c[8:, :-8] + c[:-8, :-8])[::step, ::step]

    return boxes(x), boxes(y), boxes(x * x + y * y), boxes(x * y)


def quotients(a: np.ndarray, b: np.ndarray, mutant=None) -> np.ndarray:
    """Q_c of every window: (rows, columns, 4) int64."""
    s1, s2, ss, s12 = window_sums(a, b, mutant)
    vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    n = (2 * s1 * s2 + 416) * (2 * covar + 235963)
    d = (s1 * s1 + s2 * s2 + 416) * (vars_ + 235963)
    if mutant == "narrow_n":
        n = n.astype(np.int32).astype(np.int64)
    if mutant == "narrow_d":
        d = np.maximum(d.astype(np.uint32).astype(np.int64), 1)
    out = np.empty(n.size, np.int64)
    for i, (ni, di) in enumerate(zip(n.reshape(-1).tolist(), d.reshape(-1).tolist())):
        q = (2 * (abs(ni) << 24) + di) // (2 * di) if mutant == "round" else (abs(ni) << 24) // di
        q = min(q, ONE)                                                      # (a mutant's D may be below |N|)
        out[i] = -q if ni < 0 else q
    return out.reshape(n.shape)


def frame_ssim(a: np.ndarray, b: np.ndarray, mask: int = 0xF, mutant=None):
    assert mutant is None or mutant in MUTANTS
    return record(quotients(a, b, mutant), mask, mutant)


def record(q: np.ndarray, mask: int = 0xF, mutant=None):
    """The record under `mask` from the quotients of every window (which do not depend on the mask)."""
    assert 1 <= mask <= 15
    rows, columns = q.shape[:2]
    channels = range(4) if mutant == "hist_all" else [c for c in range(4) if mask >> c & 1]
    m = q[..., list(channels)].min(-1)                                       # the smallest Q_c over the channels of the mask
    hist = tuple(int(v) for v in np.bincount((np.maximum(m, 0) >> 18).reshape(-1), minlength=65))
    wy, wx = np.mgrid[:rows, :columns]
    order = -wx if mutant == "worst_rightmost" else wx
    at = min(zip(m.reshape(-1).tolist(), wy.reshape(-1).tolist(), order.reshape(-1).tolist()))
    worst = ((at[0] + ONE) << 32) | (at[1] << 16) | abs(at[2])
    return rows * columns, tuple(int(q[..., c].sum()) for c in range(4)), hist, worst


def add(r, s, mutant=None):
    return (r[0] if mutant == "windows_not_added" else r[0] + s[0], tuple(x + y for x, y in zip(r[1], s[1])),
            tuple(x + y for x, y in zip(r[2], s[2])), min(r[3], s[3]))


def summarize(record, mask: int = 0xF):
    windows, total, hist, worst = record
    if not 1 <= mask <= 15 or windows == 0 or sum(hist) != windows:
        return None
    ssim = tuple(total[c] / (windows * ONE) for c in range(4))               # exact integers, one rounding
    channels = [c for c in range(4) if mask >> c & 1]
    mean = 0.0
    for c in channels:
        mean += ssim[c]
    mean /= len(channels)
    return {"windows": windows, "identical": hist[64], "below_half": sum(hist[:32]), "ssim": ssim, "all": mean,
            "db": -10.0 * math.log10(1.0 - mean) if mean < 1.0 else math.inf,
            "worst_value": ((worst >> 32) - ONE) / ONE, "worst_x": 4 * (worst & 0xFFFF), "worst_y": 4 * (worst >> 16 & 0xFFFF)}


def float64_formula(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The definition's N / D in float64, per window and channel: what the integer quotient is held against."""
    s1, s2, ss, s12 = (v.astype(np.float64) for v in window_sums(a, b))      # every sum is exact in a double
    vars_, covar = 64.0 * ss - s1 * s1 - s2 * s2, 64.0 * s12 - s1 * s2       # exact: below 2^31
    return ((2.0 * s1 * s2 + 416.0) * (2.0 * covar + 235963.0)) / ((s1 * s1 + s2 * s2 + 416.0) * (vars_ + 235963.0))


# ---- the scenes

def checkerboard(w: int, h: int):
    """(a, b): a checkerboard of single pixels, 0 and 255, against its inverse."""
    yy, xx = np.mgrid[:h, :w]
    a = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 4, axis=-1)
    return a, 255 - a


def half_and_half(w: int, h: int, seed: int = 5):
    """(a, b): block columns of 0 and of 255 in turn, so every window is half 0 and half 255 -- s1^2 + s2^2 and vars at their
    largest together, D = 2^54 -- and b differs from a by one level on a tenth of the bytes, so N is not D."""
    a = np.repeat(np.tile((((np.arange(w) >> 2) & 1) * 255).astype(np.uint8), (h, 1))[..., None], 4, axis=-1)
    flip = np.random.default_rng(seed).random((h, w, 4)) < 0.1
    return a, np.where(flip, a ^ 1, a).astype(np.uint8)


def scenes(w: int, h: int):
    """{name: (a, b)} at w x h: the contents every size of the GPU tests takes, and the CPU tests hold the mutants to."""
    rng = np.random.default_rng(1000 * w + h)
    a = cases.textured(w, h, 3)
    return {"graded": dm.graded_of(w, h), "identical": (a, a.copy()),
            "0-against-255": (np.zeros((h, w, 4), np.uint8), np.full((h, w, 4), 255, np.uint8)),
            "checkerboard": checkerboard(w, h), "half-and-half": half_and_half(w, h),
            "unrelated": (rng.integers(0, 256, (h, w, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8))}
