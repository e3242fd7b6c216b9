"""CPU model of lfg_interpolate_compensated_bidirectional and lfg_motion_consistency (include/linuxfg_hip.h): the forward-backward
check, the two `confirmed` predicates, both projections, the hole fill with its symmetric revealed / covered rule and the
sampling, in the header's fp32 operation order.  The loops are C (tests/bidir_model.c, built here with the system C compiler and
-ffp-contract=off on first use); what this wrapper shares with the family's other three is in tests/c_model.py.

``consistency(a, b, tolerance)`` is lfg_motion_consistency's mask.  ``keys(prev, curr, fwd, bwd, t, ...)`` is the key image of
both projections (``which`` = "forward" / "backward" for one alone), ``sample(..., K, ...)`` the sampling step from any key
image, and ``interpolate_bidirectional(...)`` the whole frame, or with ``roi=(x, y, w, h)`` only the ROI's pixels (the
projections still cover the whole frame)."""
from __future__ import annotations

import numpy as np

from tests.c_model import DEFAULT_MATCH_SAD, HOLE          # public names of this module too
from tests.c_model import F, I, VP, frames_and_vectors as _inputs, mutant_loader, plane as _plane, ptr as _ptr
from tests.c_model import sampling as _sampling

MUTANTS = ("NEG128_AS_127", "CHEBYSHEV", "STRICT")   # bidir_model.c: what a case of test_bidir_model.py must tell from the model
_WHICH = {"forward": 1, "backward": 2, "both": 3}
_load = mutant_loader("bidir_model", {"bidir_consistency": [VP, VP, I, I, I, VP],
                                      "bidir_project": [VP, VP, VP, VP, I, I, F, I, I, I, VP],
                                      "bidir_sample": [VP, VP, VP, VP, VP, I, I, F, I, I, I, I, I, I, VP]}, "BIDIR_MUTANT_", MUTANTS)


def _field(v, shape):
    return _plane(v, np.int8, tuple(shape) + (2,))


def consistency(a: np.ndarray, b: np.ndarray, tolerance: int, mutant=None) -> np.ndarray:
    """(H, W) uint8: 255 where q + a(q) is inside and |a(q) + b(q + a(q))| in L1 is at most `tolerance`, else 0."""
    a = _field(a, np.asarray(a).shape[:2])
    b = _field(b, a.shape[:2])
    H, W = a.shape[:2]
    out = np.empty((H, W), np.uint8)
    _load(mutant).bidir_consistency(_ptr(a), _ptr(b), W, H, int(tolerance), _ptr(out))
    return out


def keys(prev, curr, fwd, bwd, t: float, match_sad: int = DEFAULT_MATCH_SAD, tolerance: int = 1, which: str = "both",
         mutant=None) -> np.ndarray:
    """(H, W) uint32: the smallest projected key of every pixel, HOLE where nothing lands."""
    prev, curr, fwd = _inputs(prev, curr, fwd)
    bwd = _field(bwd, prev.shape[:2])
    H, W = prev.shape[:2]
    K = np.empty((H, W), np.uint32)
    _load(mutant).bidir_project(_ptr(prev), _ptr(curr), _ptr(fwd), _ptr(bwd), W, H, float(t), int(match_sad), int(tolerance),
                                _WHICH[which], _ptr(K))
    return K


def sample(prev, curr, fwd, bwd, K, t: float, match_sad: int = DEFAULT_MATCH_SAD, tolerance: int = 1, roi=None,
           mutant=None) -> np.ndarray:
    """The sampling step alone, from a key image K (H, W) uint32 given by the caller: lets a test place keys and holes."""
    prev, curr, fwd = _inputs(prev, curr, fwd)
    bwd = _field(bwd, prev.shape[:2])
    H, W = prev.shape[:2]
    K, rect, out = _sampling(K, H, W, roi)
    _load(mutant).bidir_sample(_ptr(prev), _ptr(curr), _ptr(fwd), _ptr(bwd), _ptr(K), W, H, float(t), int(match_sad),
                               int(tolerance), *rect, _ptr(out))
    return out


def interpolate_bidirectional(prev, curr, fwd, bwd, t: float, match_sad: int = DEFAULT_MATCH_SAD, tolerance: int = 1, roi=None,
                              mutant=None) -> np.ndarray:
    """(H, W, 4) uint8 of the whole frame, or (h, w, 4) of roi = (x, y, w, h)."""
    K = keys(prev, curr, fwd, bwd, t, match_sad, tolerance, "both", mutant)
    return sample(prev, curr, fwd, bwd, K, t, match_sad, tolerance, roi, mutant)
