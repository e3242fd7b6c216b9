"""CPU model of lfg_motion_pyramid (include/linuxfg_hip.h): the pyramid, the level-L full search and the refinements, in
integer arithmetic exactly as the header defines them.  The inner loops are C (tests/pyramid_model.c, built here with the
system C compiler on first use): the refinements' per-pixel candidate sets do not vectorise in numpy.

``motion_pyramid(prev, curr, L, Rc, Rr)`` gives the whole frame's vectors; ``motion_pyramid(..., roi=(x, y, w, h))`` only the
ROI's, computing each level's vectors just for the ROI's ancestors there (the pyramid images are still made whole), so ROIs
of a 4K frame are cheap."""
from __future__ import annotations

import ctypes

import numpy as np

from tests.c_model import load, ptr as _ptr

_VP, _I = ctypes.c_void_p, ctypes.c_int
_SIGNATURES = {"pyramid_level": [_VP, _I, _I, _VP, _I, _I],
               "pyramid_vectors": [_VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _I, _I, _VP]}


def _load():
    return load("pyramid_model", _SIGNATURES)


def level_sizes(w: int, h: int, levels: int):
    """[(W_0, H_0), ..., (W_L, H_L)] with W_k = ceil(W_{k-1} / 2)."""
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def reduce(img: np.ndarray) -> np.ndarray:
    """One pyramid step: each channel (sum of the 2 x 2 texels, coordinates clamped, + 2) >> 2."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    out = np.empty(((H + 1) // 2, (W + 1) // 2, 4), np.uint8)
    _load().pyramid_level(_ptr(img), W, H, _ptr(out), out.shape[1], out.shape[0])
    return out


def pyramid(img: np.ndarray, levels: int):
    out = [np.ascontiguousarray(img, np.uint8)]
    for _ in range(levels):
        out.append(reduce(out[-1]))
    return out


def motion_pyramid(prev: np.ndarray, curr: np.ndarray, levels: int = 2, coarse_radius: int = 16, refine_radius: int = 2,
                   roi=None) -> np.ndarray:
    """(H, W, 2) int8 vectors (x, y) of the whole frame, or (h, w, 2) of roi = (x, y, w, h)."""
    lib = _load()
    P, C = pyramid(prev, levels), pyramid(curr, levels)
    H0, W0 = prev.shape[:2]
    x, y, w, h = roi if roi is not None else (0, 0, W0, H0)
    rects = [(x, y, x + w, y + h)]                      # [x0, x1) x [y0, y1) per level: the ROI's ancestors
    for _ in range(levels):
        a0, b0, a1, b1 = rects[-1]
        rects.append((a0 // 2, b0 // 2, (a1 - 1) // 2 + 1, (b1 - 1) // 2 + 1))
    parent = None
    for k in range(levels, -1, -1):
        x0, y0, x1, y1 = rects[k]
        Hk, Wk = P[k].shape[:2]
        out = np.empty((y1 - y0, x1 - x0, 2), np.int8)
        if parent is None:
            lib.pyramid_vectors(_ptr(P[k]), _ptr(C[k]), Wk, Hk, x0, y0, x1, y1, None, 0, coarse_radius, _ptr(out))
        else:
            lib.pyramid_vectors(_ptr(P[k]), _ptr(C[k]), Wk, Hk, x0, y0, x1, y1, _ptr(parent), parent.shape[1], refine_radius, _ptr(out))
        parent = out
    return parent


def parameters_ok(levels: int, coarse_radius: int, refine_radius: int) -> bool:
    return (1 <= levels <= 4 and 1 <= coarse_radius <= 32 and 1 <= refine_radius <= 4
            and coarse_radius * 2 ** levels + refine_radius * (2 ** levels - 1) <= 127)
