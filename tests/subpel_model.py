"""CPU model of lfg_motion_subpel and lfg_interpolate_compensated_subpel (include/linuxfg_hip.h): the fractional sample and the
two-stage quarter-pixel search; the fractional gate, the projection with its 64-bit key, the hole fill and the sampling, in the
header's operation order.  The loops are C (tests/subpel_model.c, built here with the system C compiler and
-ffp-contract=off on first use).

``refine(prev, curr, mv, radius)`` is lfg_motion_subpel: (H, W, 2) int16 in quarter pixels from (H, W, 2) int8.
``interpolate(prev, curr, mvq, t, match_sad)`` is lfg_interpolate_compensated_subpel; ``keys(...)`` the projected key image
(uint64) and ``sample(..., K, ...)`` the sampling step from any key image.  ``gate(prev, curr, mvq, match_sad)`` is the
fractional match gate alone, as a boolean image."""
from __future__ import annotations

import numpy as np

from tests.c_model import DEFAULT_MATCH_SAD, F, I, VP, mutant_loader, plane, ptr as _ptr

HOLE = 0xFFFFFFFFFFFFFFFF
LIMIT = 508
MUTANTS = ("SHORTEST_W", "ROUND_SHIFT", "ROUND_7", "STAGE2_AT_4V")     # subpel_model.c: what the shared cases must tell from the model
_load = mutant_loader("subpel_model", {"subpel_refine": [VP, VP, VP, I, I, I, VP],
                                       "subpel_project": [VP, VP, VP, I, I, F, I, VP],
                                       "subpel_sample": [VP, VP, VP, VP, I, I, F, I, I, I, I, I, VP]}, "SUBPEL_MUTANT_", MUTANTS)


def key(wx: int, wy: int) -> int:
    """A clamped quarter-pixel vector's projection key: the smallest key wins (longest, then smallest wy, then smallest wx)."""
    return ((0xFFFFF - (wx * wx + wy * wy)) << 20) | ((wy + 512) << 10) | (wx + 512)


def _frames(prev, curr):
    prev = np.ascontiguousarray(prev, np.uint8)
    assert prev.ndim == 3 and prev.shape[2] == 4, prev.shape
    return prev, plane(curr, np.uint8, prev.shape)


def refine(prev, curr, mv, radius: int, mutant=None) -> np.ndarray:
    prev, curr = _frames(prev, curr)
    H, W = prev.shape[:2]
    mv = plane(mv, np.int8, (H, W, 2))
    out = np.empty((H, W, 2), np.int16)
    _load(mutant).subpel_refine(_ptr(prev), _ptr(curr), _ptr(mv), W, H, int(radius), _ptr(out))
    return out


def keys(prev, curr, mvq, t: float, match_sad: int = DEFAULT_MATCH_SAD, mutant=None) -> np.ndarray:
    """(H, W) uint64: the projected key of every pixel, HOLE where nothing lands."""
    prev, curr = _frames(prev, curr)
    H, W = prev.shape[:2]
    mvq = plane(mvq, np.int16, (H, W, 2))
    K = np.empty((H, W), np.uint64)
    _load(mutant).subpel_project(_ptr(prev), _ptr(curr), _ptr(mvq), W, H, float(t), int(match_sad), _ptr(K))
    return K


def sample(prev, curr, mvq, K, t: float, match_sad: int = DEFAULT_MATCH_SAD, mutant=None) -> np.ndarray:
    prev, curr = _frames(prev, curr)
    H, W = prev.shape[:2]
    mvq, K = plane(mvq, np.int16, (H, W, 2)), plane(K, np.uint64, (H, W))
    out = np.empty((H, W, 4), np.uint8)
    _load(mutant).subpel_sample(_ptr(prev), _ptr(curr), _ptr(mvq), _ptr(K), W, H, float(t), int(match_sad), 0, 0, W, H, _ptr(out))
    return out


def interpolate(prev, curr, mvq, t: float, match_sad: int = DEFAULT_MATCH_SAD, mutant=None) -> np.ndarray:
    return sample(prev, curr, mvq, keys(prev, curr, mvq, t, match_sad, mutant), t, match_sad, mutant)


def gate(prev, curr, mvq, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    """(H, W) bool: the pixels that pass the fractional gate.  At t = 1 a matched pixel projects onto itself and nothing else
    lands anywhere, so the key image of t = 1 is the gate."""
    return keys(prev, curr, mvq, 1.0, match_sad) != np.uint64(HOLE)
