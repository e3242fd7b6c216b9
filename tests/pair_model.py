"""CPU model of lfg_pair_match and lfg_cut_fallback, restated in numpy from include/linuxfg_hip.h (not from tests/mc_model.c,
whose gate it is held to in tests/test_pair_model.py).

``sad_map(prev, curr, mv)`` is sad(q) of every pixel, ``pair_stats(prev, curr, mv, match_sad)`` the record (pixels, matched,
sad_sum) in Python integers, ``cut(stats, permille)`` the decision of lfg_cut_fallback and ``fallback(prev, curr, factors)``
the frames it writes on a cut."""
from __future__ import annotations

import numpy as np


def sad_map(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray) -> np.ndarray:
    """(H, W) int64: sum over the channels of |curr(q) - prev(q + mv(q))|, prev outside the image read as 0."""
    h, w = curr.shape[:2]
    assert prev.shape == curr.shape == (h, w, 4) and mv.shape == (h, w, 2) and mv.dtype == np.int8
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs + mv[..., 0].astype(np.int64), ys + mv[..., 1].astype(np.int64)
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    fetched = np.zeros((h, w, 4), np.int64)
    fetched[inside] = prev[sy[inside], sx[inside]]
    return np.abs(curr.astype(np.int64) - fetched).sum(-1)


def matched_mask(prev, curr, mv, match_sad: int) -> np.ndarray:
    return sad_map(prev, curr, mv) <= int(match_sad)


def pair_stats(prev, curr, mv, match_sad: int):
    """(pixels, matched, sad_sum) as lfg_pair_match writes them."""
    sad = sad_map(prev, curr, mv)
    return int(sad.size), int((sad <= int(match_sad)).sum()), int(sad.sum())


def permille(stats) -> int:
    """Matched pixels per thousand, rounded down: reporting only, the decision is cut()."""
    pixels, matched, _ = stats
    return matched * 1000 // pixels


def cut(stats, min_matched_permille: int) -> bool:
    """matched * 1000 < min_matched_permille * pixels, in exact integers; 0 never cuts."""
    pixels, matched, _ = stats
    return int(matched) * 1000 < int(min_matched_permille) * int(pixels)


def takes_curr(factor) -> bool:
    """Which source an output of a cut shows: prev where the fp32 factor is below 0.5f, curr otherwise."""
    return not bool(np.float32(factor) < np.float32(0.5))


def fallback(prev, curr, factors):
    """The frames lfg_cut_fallback leaves on a cut, one per factor (shared with the inputs: compare, do not write)."""
    return [curr if takes_curr(t) else prev for t in factors]
