"""CPU model of lfg_interpolate_compensated (include/linuxfg_hip.h): the match gate, the projection of the vectors to time t,
the hole fill and the sampling, in the header's fp32 operation order.  The loops are C (tests/mc_model.c, built here with
the system C compiler and -ffp-contract=off on first use); what this wrapper shares with the family's other three is in
tests/c_model.py.

``interpolate_compensated(prev, curr, mv, t, match_sad)`` gives the whole frame; ``..., roi=(x, y, w, h)`` only the ROI's
pixels (the projection still covers the whole frame: any source pixel may land in the ROI), so ROIs of a 4K or 8K frame are
cheap.  ``keys(...)`` is the projected key image itself, and ``sample(..., K, ...)`` the sampling step from any key image."""
from __future__ import annotations

import numpy as np

from tests.c_model import DEFAULT_MATCH_SAD, HOLE, key     # public names of this module too
from tests.c_model import F, I, VP, frames_and_vectors as _inputs, mutant_loader, ptr as _ptr, sampling as _sampling

MUTANTS = ("C_FROM_P", "CEIL_PROJECT", "HALF_LAST")     # mc_model.c: rewrites that a test's factors must tell from the model
_load = mutant_loader("mc_model", {"mc_project": [VP, VP, VP, I, I, F, I, VP],
                                   "mc_sample": [VP, VP, VP, VP, I, I, F, I, I, I, I, I, VP]}, "MC_MUTANT_", MUTANTS)


def keys(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray, t: float, match_sad: int = DEFAULT_MATCH_SAD,
         mutant=None) -> np.ndarray:
    """(H, W) uint32: the projected key of every pixel, HOLE where nothing lands."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K = np.empty((H, W), np.uint32)
    _load(mutant).mc_project(_ptr(prev), _ptr(curr), _ptr(mv), W, H, float(t), int(match_sad), _ptr(K))
    return K


def interpolate_compensated(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray, t: float,
                            match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """(H, W, 4) uint8 of the whole frame, or (h, w, 4) of roi = (x, y, w, h)."""
    return sample(prev, curr, mv, keys(prev, curr, mv, t, match_sad, mutant), t, match_sad, roi, mutant)


def sample(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray, K: np.ndarray, t: float,
           match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """The sampling step alone, from a key image K (H, W) uint32 given by the caller: lets a test place keys and holes."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K, rect, out = _sampling(K, H, W, roi)
    _load(mutant).mc_sample(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(K), W, H, float(t), int(match_sad), *rect, _ptr(out))
    return out


def moving_square(w: int = 96, h: int = 64, size: int = 16, at=(30, 24), shift=(12, 0), seed: int = 7):
    """A textured size x size square that moves by `shift` over a static textured background: (prev, curr, square's
    top-left in prev).  The textures are uncorrelated noise, so the block matcher finds both motions."""
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    sq = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
    x, y = at
    prev = bg.copy()
    prev[y:y + size, x:x + size] = sq
    curr = bg.copy()
    curr[y + shift[1]:y + shift[1] + size, x + shift[0]:x + shift[0] + size] = sq
    return prev, curr, (x, y)
