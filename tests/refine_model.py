"""CPU model of lfg_motion_refine (include/linuxfg_hip.h): for each pixel, the candidate vector of the 17 positions around it
with the smallest key (window cost, |v|^2, vy, vx).  The loops are C (tests/refine_model.c, built here with the system C
compiler on first use).

``refine(prev, curr, mv, radius)`` gives the whole frame's vectors; ``refine(..., roi=(x, y, w, h))`` only the ROI's (each
output depends only on mv within 8 px and the frames within radius + 128 px), so ROIs of a 4K or 8K frame are cheap.
``candidates(mv, x, y)`` lists a pixel's candidates."""
from __future__ import annotations

import ctypes

import numpy as np

from linux_fg_amd import synth
from tests.c_model import frames_and_vectors, load, ptr as _ptr

_VP, _I = ctypes.c_void_p, ctypes.c_int
_SIGNATURES = {"refine_roi": [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _I, _VP]}

# candidate offsets: (0, 0), then s = 4, 8, then b, then a, skipping (a, b) = (0, 0)
OFFSETS = [(0, 0)] + [(a * s, b * s) for s in (4, 8) for b in (-1, 0, 1) for a in (-1, 0, 1) if (a, b) != (0, 0)]


def refine(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray, radius: int = 1, roi=None) -> np.ndarray:
    """(H, W, 2) int8 of the whole frame, or (h, w, 2) of roi = (x, y, w, h)."""
    prev, curr, mv = frames_and_vectors(prev, curr, mv)
    assert 0 <= radius <= 2
    H, W = prev.shape[:2]
    x, y, w, h = roi if roi is not None else (0, 0, W, H)
    out = np.empty((h, w, 2), np.int8)
    load("refine_model", _SIGNATURES).refine_roi(_ptr(prev), _ptr(curr), _ptr(mv), W, H, int(radius), x, y, x + w, y + h, _ptr(out))
    return out


def candidates(mv: np.ndarray, x: int, y: int):
    """The candidate vectors (vx, vy) of pixel (x, y): mv at every offset that stays inside the image."""
    H, W = mv.shape[:2]
    return [tuple(int(c) for c in mv[y + dy, x + dx]) for dx, dy in OFFSETS if 0 <= x + dx < W and 0 <= y + dy < H]


def moving_objects(w: int = 640, h: int = 360, pan=(4, -2), squares=((24, (200, 120), (10, 6)), (40, (380, 200), (-14, 4))),
                   margin: int = 8, seed: int = 11):
    """A synth background panned by `pan` and textured squares (size, top-left in prev, shift) moving over it.  Returns
    (prev, curr, truth, mid, band): truth the (H, W, 2) true vectors of curr (prev(q + v) = curr(q)), mid the true frame
    at t = 0.5 (shifts even), band the pixels within `margin` px of a square's edge in prev, at t = 0.5 or in curr."""
    rng = np.random.default_rng(seed)
    bg = synth.make_prev(w, h, synth.BASE_SEED + seed)
    prev = bg.copy()
    curr = synth.translate(bg, pan, synth.BASE_SEED + seed)
    mid = synth.translate(bg, (pan[0] // 2, pan[1] // 2), synth.BASE_SEED + seed)
    truth = np.zeros((h, w, 2), np.int8)
    truth[...] = (-pan[0], -pan[1])
    band = np.zeros((h, w), bool)
    for size, (x, y), (sx, sy) in squares:
        tex = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
        prev[y:y + size, x:x + size] = tex
        curr[y + sy:y + sy + size, x + sx:x + sx + size] = tex
        mid[y + sy // 2:y + sy // 2 + size, x + sx // 2:x + sx // 2 + size] = tex
        truth[y + sy:y + sy + size, x + sx:x + sx + size] = (-sx, -sy)
        for ox, oy in ((x, y), (x + sx // 2, y + sy // 2), (x + sx, y + sy)):
            outer = np.zeros((h, w), bool)
            outer[max(0, oy - margin):oy + size + margin, max(0, ox - margin):ox + size + margin] = True
            outer[oy + margin + 1:oy + size - margin - 1, ox + margin + 1:ox + size - margin - 1] = False
            band |= outer
    return prev, curr, truth, mid, band
