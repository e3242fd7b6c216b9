"""CPU model of lfg_static_mask and lfg_interpolate_compensated_masked (include/linuxfg_hip.h).  The mask is numpy; the
masked interpolation's loops are C (tests/overlay_model.c, built on first use with the system C compiler and
-ffp-contract=off, like tests/mc_model.py).

``static_mask(prev, curr, tolerance)`` is the (H, W) uint8 mask, 255 where the pair is static.
``interpolate_masked(prev, curr, mv, mask, t, match_sad)`` gives the whole frame, ``..., roi=(x, y, w, h)`` the ROI's pixels;
``keys(...)`` the projected key image (0 at every static location) and ``sample(..., K, ...)`` the sampling from any key
image."""
from __future__ import annotations

import ctypes

import numpy as np

from tests.c_model import frames_and_vectors as _inputs, load, ptr as _ptr

_VP, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_SIGNATURES = {"ov_project": [_VP, _VP, _VP, _VP, _I, _I, _F, _I, _VP],
               "ov_sample": [_VP, _VP, _VP, _VP, _VP, _I, _I, _F, _I, _I, _I, _I, _I, _VP]}

HOLE = 0xFFFFFFFF
STATIC = 0
DEFAULT_MATCH_SAD = 48
# overlay_model.c: what the shared cases must tell from the model
MUTANTS = ("NO_PROJECT", "WALK_STOPS", "RULE_AFTER_HOLE", "RULE_LRINT", "STATIC_CURR")


def _load(mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    return load("overlay_model", _SIGNATURES, ["-ffp-contract=off"] + ([f"-DOV_MUTANT_{mutant}"] if mutant else []), ["-lm"])


def static_mask(prev: np.ndarray, curr: np.ndarray, tolerance: int = 0) -> np.ndarray:
    """lfg_static_mask: 255 where the sum over the four channels of |prev - curr| is at most `tolerance`, else 0."""
    sad = np.abs(prev.astype(np.int16) - curr.astype(np.int16)).sum(-1)
    return np.where(sad <= int(tolerance), 255, 0).astype(np.uint8)


def _mask(mask, shape):
    mask = np.ascontiguousarray(mask, np.uint8)
    assert mask.shape == shape, (mask.shape, shape)
    return mask


def keys(prev, curr, mv, mask, t: float, match_sad: int = DEFAULT_MATCH_SAD, mutant=None) -> np.ndarray:
    """(H, W) uint32: the projected key of every pixel, HOLE where nothing lands, STATIC (0) where the mask is set."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K = np.empty((H, W), np.uint32)
    _load(mutant).ov_project(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(_mask(mask, (H, W))), W, H, float(t), int(match_sad), _ptr(K))
    return K


def sample(prev, curr, mv, mask, K, t: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """The sampling step alone, from a key image K (H, W) uint32 given by the caller."""
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    K = np.ascontiguousarray(K, np.uint32)
    assert K.shape == (H, W)
    x, y, w, h = roi if roi is not None else (0, 0, W, H)
    out = np.empty((h, w, 4), np.uint8)
    _load(mutant).ov_sample(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(_mask(mask, (H, W))), _ptr(K), W, H, float(t), int(match_sad),
                            x, y, x + w, y + h, _ptr(out))
    return out


def interpolate_masked(prev, curr, mv, mask, t: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, mutant=None) -> np.ndarray:
    """(H, W, 4) uint8 of the whole frame, or (h, w, 4) of roi = (x, y, w, h)."""
    return sample(prev, curr, mv, mask, keys(prev, curr, mv, mask, t, match_sad, mutant), t, match_sad, roi, mutant)
