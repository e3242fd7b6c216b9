"""CPU model of lfg_frame_diff and lfg_frame_diff_summarize, restated in numpy and Python integers from include/linuxfg_hip.h
(not from csrc/frame_diff.hip), and the graded inputs that the CPU and GPU tests of the comparison share.

``frame_diff(a, b, mask)`` is the record (pixels, sse tuple of 4, hist tuple of 256) as lfg_frame_diff writes it,
``add(r, s)`` the word-wise sum of two records (what accumulate = 1 gives), ``summarize(record, mask)`` the dict of
lfg_frame_diff_summarize's figures, or None where the call returns LFG_ERR_INVALID."""
from __future__ import annotations

import math

import numpy as np

from tests import cases

MASKS = (0xF, 0x7, 0x8, 0x5)


def frame_diff(a: np.ndarray, b: np.ndarray, mask: int = 0xF):
    assert a.shape == b.shape and a.shape[2] == 4 and a.dtype == b.dtype == np.uint8 and 1 <= mask <= 15
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))                      # d_c(q)
    sse = tuple(int((d[..., c] ** 2).sum()) for c in range(4))
    m = d[..., [c for c in range(4) if mask >> c & 1]].max(-1)               # the largest d_c over the channels of the mask
    hist = tuple(int(v) for v in np.bincount(m.reshape(-1), minlength=256))
    return a.shape[0] * a.shape[1], sse, hist


def add(r, s):
    return r[0] + s[0], tuple(x + y for x, y in zip(r[1], s[1])), tuple(x + y for x, y in zip(r[2], s[2]))


def summarize(record, mask: int = 0xF):
    pixels, sse, hist = record
    if not 1 <= mask <= 15 or pixels == 0 or sum(hist) != pixels:
        return None
    differing = pixels - hist[0]

    def quantile(p):
        below = 0
        for k in range(256):
            below += hist[k]
            if 100 * below >= p * pixels:
                return k
        raise AssertionError("unreachable: the histogram sums to pixels")

    channels = [c for c in range(4) if mask >> c & 1]
    mse = sum(sse[c] for c in channels) / (len(channels) * pixels)           # exact integers, one rounding
    return {"pixels": pixels, "differing": differing, "over_1": differing - hist[1],
            "max_abs": max((k for k in range(256) if hist[k] > 0), default=0), "p50": quantile(50), "p99": quantile(99),
            "mse": mse, "psnr_db": 10.0 * math.log10(65025.0 / mse) if mse > 0 else math.inf}


# ---- the graded inputs

def graded(w: int, h: int, seed: int):
    """(a, b): a is textured; per pixel b is, with probabilities 0.4 / 0.3 / 0.2 / 0.1, equal to a, a with +-1 on one random
    channel (clipped), a within +-14 per channel (clipped), or unrelated texture.  Then the first pixel is 0 in a and 255 in
    b, the last 255 in a and 0 in b: bins 0, 1 and 255 are populated at any size of two pixels or more."""
    a = cases.textured(w, h, seed).copy()
    rng = np.random.default_rng(seed + 7000)
    grade = rng.choice(4, size=(h, w), p=[0.4, 0.3, 0.2, 0.1])
    wide = a.astype(np.int16)
    one = np.zeros((h, w, 4), np.int16)
    np.put_along_axis(one, rng.integers(0, 4, (h, w, 1)), rng.choice([-1, 1], size=(h, w, 1)).astype(np.int16), axis=-1)
    near = np.clip(wide + one, 0, 255).astype(np.uint8)
    mid = np.clip(wide + rng.integers(-14, 15, (h, w, 4)), 0, 255).astype(np.uint8)
    b = np.select([(grade == g)[..., None] for g in range(4)], [a, near, mid, cases.textured(w, h, seed + 1)]).astype(np.uint8)
    a.reshape(-1, 4)[0], b.reshape(-1, 4)[0] = 0, 255
    a.reshape(-1, 4)[-1], b.reshape(-1, 4)[-1] = 255, 0
    return a, b


def graded_of(w: int, h: int):
    """The graded pair that the CPU test of its power and the GPU tests both take at w x h."""
    return graded(w, h, 1000 * w + h)
