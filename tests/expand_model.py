"""CPU model of lfg_frame_halve and lfg_motion_expand (include/linuxfg_hip.h).  The loops are C (tests/expand_model.c, built
here with the system C compiler on first use).

``halve(img)`` gives the ceil(W / 2) x ceil(H / 2) frame.  ``expand(prev, curr, mv_low, radius)`` gives the whole frame's
vectors; ``expand(..., roi=(x, y, w, h))`` only the ROI's (each output depends only on mv_low within one texel of its own
and on the frames within radius + 129 px).  ``expand(..., mutant=name)`` runs one of the deliberate departures listed in the C
source."""
from __future__ import annotations

import ctypes

import numpy as np

from tests.c_model import load, plane, ptr as _ptr

_VP, _I = ctypes.c_void_p, ctypes.c_int
_SIGNATURES = {"expand_halve": [_VP, _I, _I, _VP], "expand_roi": [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _I, _VP]}
MUTANTS = ("NO_SATURATION", "NO_PARITY", "NEIGHBOURS_2X2", "ROUND_UP", "TIE_VX_FIRST")


def _load(mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    return load("expand_model", _SIGNATURES, [f"-DEXPAND_MUTANT_{mutant}"] if mutant else [])


def low_size(w: int, h: int):
    return (w + 1) // 2, (h + 1) // 2


def halve(img: np.ndarray) -> np.ndarray:
    """Each channel (sum of the 2 x 2 texels, coordinates clamped, + 2) >> 2."""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 4, img.shape
    H, W = img.shape[:2]
    wl, hl = low_size(W, H)
    out = np.empty((hl, wl, 4), np.uint8)
    _load().expand_halve(_ptr(img), W, H, _ptr(out))
    return out


def expand(prev: np.ndarray, curr: np.ndarray, mv_low: np.ndarray, radius: int = 1, roi=None, mutant=None) -> np.ndarray:
    """(H, W, 2) int8 of the whole frame, or (h, w, 2) of roi = (x, y, w, h)."""
    prev = np.ascontiguousarray(prev, np.uint8)
    assert prev.ndim == 3 and prev.shape[2] == 4, prev.shape
    H, W = prev.shape[:2]
    curr = plane(curr, np.uint8, prev.shape)
    wl, hl = low_size(W, H)
    mv_low = plane(mv_low, np.int8, (hl, wl, 2))
    assert 0 <= radius <= 2
    x, y, w, h = roi if roi is not None else (0, 0, W, H)
    out = np.empty((h, w, 2), np.int8)
    _load(mutant).expand_roi(_ptr(prev), _ptr(curr), _ptr(mv_low), W, H, int(radius), x, y, x + w, y + h, _ptr(out))
    return out
