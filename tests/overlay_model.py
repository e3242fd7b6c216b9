"""CPU model of lfg_static_mask and lfg_interpolate_compensated_masked (include/linuxfg_hip.h).  The mask is numpy; the
masked interpolation's loops are C (tests/overlay_model.c, built on first use with the system C compiler and
-ffp-contract=off); what this wrapper shares with the family's other three is in tests/c_model.py.

``static_mask(prev, curr, tolerance)`` is the (H, W) uint8 mask, 255 where the pair is static.
``interpolate_masked(prev, curr, mv, mask, t, match_sad)`` gives the whole frame, ``..., roi=(x, y, w, h)`` the ROI's pixels;
``keys(...)`` the projected key image (0 at every static location) and ``sample(..., K, ...)`` the sampling from any key
image."""
from __future__ import annotations

import numpy as np

from tests.c_model import DEFAULT_MATCH_SAD, HOLE          # public names of this module too
from tests.c_model import F, I, VP, frames_and_vectors as _inputs, mutant_loader, plane as _plane, ptr as _ptr
from tests.c_model import sampling as _sampling

STATIC = 0
# overlay_model.c: what the shared cases must tell from the model
MUTANTS = ("NO_PROJECT", "WALK_STOPS", "RULE_AFTER_HOLE", "RULE_LRINT", "STATIC_CURR")
_load = mutant_loader("overlay_model", {"ov_project": [VP, VP, VP, VP, I, I, F, I, VP],
                                        "ov_sample": [VP, VP, VP, VP, VP, I, I, F, I, I, I, I, I, VP]}, "OV_MUTANT_", MUTANTS)


def static_mask(prev: np.ndarray, curr: np.ndarray, tolerance: int = 0) -> np.ndarray:
    """lfg_static_mask: 255 where the sum over the four channels of |prev - curr| is at most `tolerance`, else 0."""
    sad = np.abs(prev.astype(np.int16) - curr.astype(np.int16)).sum(-1)
    return np.where(sad <= int(tolerance), 255, 0).astype(np.uint8)


def keys(prev, curr, mv, mask, t: float, match_sad: int = DEFAULT_MATCH_SAD, mutant=None) -> np.ndarray:
    """(H, W) uint32: the projected key of every pixel, HOLE where nothing lands, STATIC (0) where the mask is set."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K = np.empty((H, W), np.uint32)
    _load(mutant).ov_project(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(_plane(mask, np.uint8, (H, W))), W, H, float(t), int(match_sad),
                             _ptr(K))
    return K


def sample(prev, curr, mv, mask, K, t: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """The sampling step alone, from a key image K (H, W) uint32 given by the caller."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K, rect, out = _sampling(K, H, W, roi)
    _load(mutant).ov_sample(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(_plane(mask, np.uint8, (H, W))), _ptr(K), W, H, float(t),
                            int(match_sad), *rect, _ptr(out))
    return out


def interpolate_masked(prev, curr, mv, mask, t: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """(H, W, 4) uint8 of the whole frame, or (h, w, 4) of roi = (x, y, w, h)."""
    return sample(prev, curr, mv, mask, keys(prev, curr, mv, mask, t, match_sad, mutant), t, match_sad, roi, mutant)
