"""CPU model of the bicubic fetch and of lfg_interpolate_compensated_sampled with LFG_SAMPLING_BICUBIC (include/linuxfg_hip.h).
The loops are C (tests/bicubic_model.c, built here with the system C compiler and -ffp-contract=off on first use); the
projections are tests/mc_model.py's and tests/subpel_model.py's.

``weights()`` is the table Wt (64, 4) from the rational rule; ``body(img, i, j, phix, phiy)`` the integer body at one texel and
``fetch(img, px, py)`` one fetch as four floats.  ``interpolate(prev, curr, mv, t, match_sad)`` is the whole call: an int8 field
takes lfg_interpolate_compensated's route, an int16 one lfg_interpolate_compensated_subpel's; ``..., roi=(x, y, w, h)`` gives only
the ROI's pixels.  ``sample(..., K, ...)`` is the sampling step from any key image; with ``phases=`` a (2, 65) uint32 array it
also counts the horizontal and vertical phase of every fetch it makes."""
from __future__ import annotations

import numpy as np

from tests import mc_model, subpel_model
from tests.c_model import DEFAULT_MATCH_SAD, F, I, VP, mutant_loader, plane, ptr as _ptr

MUTANTS = ("TRUNC_SHIFT", "ROUND_PHASE", "NO_CLAMP")     # bicubic_model.c: what named cases must tell from the model
EQUIVALENT = ("WRONG_TAP",)                              # ... and the rewrite that changes nothing (tests/test_bicubic_model.py)
_SAMPLE = [VP, VP, VP, VP, I, I, F, I, I, I, I, I, VP, VP]
_load = mutant_loader("bicubic_model", {"bicubic_table": [VP], "bicubic_body": [VP, I, I, I, I, I, I, VP, VP],
                                        "bicubic_phases": [F, F, VP], "bicubic_fetch": [VP, I, I, F, F, VP],
                                        "bicubic_mc_sample": _SAMPLE, "bicubic_subpel_sample": _SAMPLE}, "BICUBIC_MUTANT_", MUTANTS + EQUIVALENT)
P_MAX = 65280


def weights(mutant=None) -> np.ndarray:
    w = np.empty((64, 4), np.int16)
    _load(mutant).bicubic_table(_ptr(w))
    return w


def _image(img):
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] == 4, img.shape
    return img


def body(img, i: int, j: int, phix: int, phiy: int, extremes=None, mutant=None) -> np.ndarray:
    """p (4,) int32 of the footprint around texel (i, j).  `extremes`, an int32 array (h min, h max, s min, s max), is widened."""
    img = _image(img)
    p = np.empty(4, np.int32)
    _load(mutant).bicubic_body(_ptr(img), img.shape[1], img.shape[0], int(i), int(j), int(phix), int(phiy), _ptr(p),
                               _ptr(extremes) if extremes is not None else None)
    return p


def phases_of(px: float, py: float, mutant=None):
    ph = np.empty(2, np.int32)
    _load(mutant).bicubic_phases(float(px), float(py), _ptr(ph))
    return int(ph[0]), int(ph[1])


def fetch(img, px: float, py: float, mutant=None) -> np.ndarray:
    img = _image(img)
    out = np.empty(4, np.float32)
    _load(mutant).bicubic_fetch(_ptr(img), img.shape[1], img.shape[0], float(px), float(py), _ptr(out))
    return out


def _subpel(mv) -> bool:
    return np.asarray(mv).dtype == np.int16


def keys(prev, curr, mv, t: float, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    """The projected key image of the route that mv's type picks: the bilinear routes' own."""
    return (subpel_model.keys if _subpel(mv) else mc_model.keys)(prev, curr, mv, t, match_sad)


def sample(prev, curr, mv, K, t: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, phases=None, mutant=None) -> np.ndarray:
    prev = _image(prev)
    H, W = prev.shape[:2]
    curr = plane(curr, np.uint8, prev.shape)
    x, y, w, h = roi if roi is not None else (0, 0, W, H)
    out = np.empty((h, w, 4), np.uint8)
    if phases is not None:
        assert phases.dtype == np.uint32 and phases.shape == (2, 65) and phases.flags.c_contiguous
    if _subpel(mv):
        mv, K, fn = plane(mv, np.int16, (H, W, 2)), plane(K, np.uint64, (H, W)), _load(mutant).bicubic_subpel_sample
    else:
        mv, K, fn = plane(mv, np.int8, (H, W, 2)), plane(K, np.uint32, (H, W)), _load(mutant).bicubic_mc_sample
    fn(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(K), W, H, float(t), int(match_sad), x, y, x + w, y + h, _ptr(out),
       _ptr(phases) if phases is not None else None)
    return out


def interpolate(prev, curr, mv, t: float, match_sad: int = DEFAULT_MATCH_SAD, roi=None, phases=None, mutant=None) -> np.ndarray:
    return sample(prev, curr, mv, keys(prev, curr, mv, t, match_sad), t, match_sad, roi, phases, mutant)


def bilinear(prev, curr, mv, t: float, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    """The same call with LFG_SAMPLING_BILINEAR: the existing models."""
    if _subpel(mv):
        return subpel_model.interpolate(prev, curr, mv, t, match_sad)
    return mc_model.interpolate_compensated(prev, curr, mv, t, match_sad)


# ---- the cases the CPU tests, the host program and the GPU tests share

def checkerboard(w: int, h: int) -> np.ndarray:
    """0 / 255 by texel: the image with the largest negative h_r."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 4, axis=2)


def step(w: int, h: int, lo: int, hi: int, at=None) -> np.ndarray:
    """A vertical edge: lo left of column `at` (default w // 2), hi from it on."""
    img = np.full((h, w, 4), lo, np.uint8)
    img[:, (w // 2 if at is None else at):] = hi
    return img
