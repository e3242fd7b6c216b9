"""CPU model of lfg_extrapolate_compensated (include/linuxfg_hip.h): the match gate, the projection of curr's vectors past
time 1, the hole walk with its donor rule and the sampling of curr, in the header's fp32 operation order.  The loops are C
(tests/extrapolate_model.c, built here with the system C compiler and -ffp-contract=off on first use); what this wrapper
shares with the family's other three is in tests/c_model.py.

``extrapolate(prev, curr, mv, a, match_sad)`` gives the whole frame; ``..., roi=(x, y, w, h)`` only the ROI's pixels (the
projection still covers the whole frame: any source pixel may land in the ROI).  ``keys(...)`` is the projected key image
itself, ``sample(..., K, ...)`` the sampling step from any key image, and ``branches(...)`` says how each pixel was made."""
from __future__ import annotations

import numpy as np

from tests.c_model import DEFAULT_MATCH_SAD, HOLE, key     # public names of this module too
from tests.c_model import F, I, VP, frames_and_vectors as _inputs, mutant_loader, ptr as _ptr, sampling as _sampling

PROJECTED, NO_DONOR, DONOR_KEPT, DONOR_TAKEN = 0, 1, 2, 3      # branches(): how a pixel was made
# extrapolate_model.c: what the shared cases (tests/extrapolate_cases.py) must tell from the model
MUTANTS = ("PLUS_V", "CEIL_PROJECT", "ONE_MINUS_A", "NO_DONOR", "LATER_TIE")
_load = mutant_loader("extrapolate_model", {"ex_project": [VP, VP, VP, I, I, F, I, VP],
                                            "ex_sample": [VP, VP, VP, VP, I, I, F, I, I, I, I, I, VP, VP]}, "EX_MUTANT_", MUTANTS)


def keys(prev, curr, mv, a: float, match_sad: int = DEFAULT_MATCH_SAD, mutant=None) -> np.ndarray:
    """(H, W) uint32: the projected key of every pixel, HOLE where nothing lands."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K = np.empty((H, W), np.uint32)
    _load(mutant).ex_project(_ptr(prev), _ptr(curr), _ptr(mv), W, H, float(a), int(match_sad), _ptr(K))
    return K


def _sample(prev, curr, mv, K, a, match_sad, roi, mutant):
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K, rect, out = _sampling(K, H, W, roi)
    how = np.empty(out.shape[:2], np.uint8)
    _load(mutant).ex_sample(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(K), W, H, float(a), int(match_sad), *rect, _ptr(out), _ptr(how))
    return out, how


def sample(prev, curr, mv, K, a: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """The sampling step alone, from a key image K (H, W) uint32 given by the caller: lets a test place keys and holes."""
    return _sample(prev, curr, mv, K, a, match_sad, roi, mutant)[0]


def extrapolate(prev, curr, mv, a: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """(H, W, 4) uint8 of the whole frame at time 1 + a, or (h, w, 4) of roi = (x, y, w, h)."""
    return sample(prev, curr, mv, keys(prev, curr, mv, a, match_sad, mutant), a, match_sad, roi, mutant)


def branches(prev, curr, mv, a: float, match_sad: int = DEFAULT_MATCH_SAD, K=None) -> np.ndarray:
    """(H, W) uint8 of PROJECTED / NO_DONOR / DONOR_KEPT / DONOR_TAKEN: how extrapolate() made each pixel."""
    return _sample(prev, curr, mv, keys(prev, curr, mv, a, match_sad) if K is None else K, a, match_sad, None, None)[1]
