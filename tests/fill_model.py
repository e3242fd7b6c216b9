"""CPU model of the fill plane (lfg_hole_fill_plane, lfg_set_hole_reach; include/linuxfg_hip.h).  The loops are C
(tests/fill_model.c, built here with the system C compiler and -ffp-contract=off on first use); the loader and the hand-over
of arrays are tests/c_model.py's.

``plane(K, reach, pass_static)`` is the plane of any key image, by plain loops from the definition.  ``sample(prev, curr, mv,
K, P, t)``, ``sample_masked(..., mask, K, P, t)`` and ``sample_bidirectional(prev, curr, fwd, bwd, K, P, t)`` are the three
sampling steps with a hole's vector read from the plane P, and ``interpolate_compensated``, ``interpolate_masked`` and
``interpolate_bidirectional`` the whole calls under lfg_set_hole_reach(reach): the projection is the existing models', which
the setting does not change.

``fast_scene(...)`` is the scene the reach was measured on: a noise square that moves fast over a panning noise background."""
from __future__ import annotations

import numpy as np

from tests import bidir_model, mc_model, overlay_model
from tests.c_model import DEFAULT_MATCH_SAD, HOLE          # public names of this module too
from tests.c_model import F, I, VP, frames_and_vectors as _inputs, mutant_loader, plane as _plane, ptr as _ptr

STATIC = 0
REACH_MAX = 255
# fill_model.c: what a plane case of test_fill_model.py must tell from the model
MUTANTS = ("STRICT_REACH", "PROJECTION_MIN", "STATIC_DONOR", "SELF_DONOR", "COLUMN_OF_PLANE")
_load = mutant_loader("fill_model", {"fill_plane": [VP, I, I, I, I, VP],
                                     "fill_mc_sample": [VP, VP, VP, VP, VP, I, I, F, I, VP],
                                     "fill_ov_sample": [VP, VP, VP, VP, VP, VP, I, I, F, I, VP],
                                     "fill_bidir_sample": [VP, VP, VP, VP, VP, VP, I, I, F, I, I, VP]}, "FILL_MUTANT_", MUTANTS)


def order(vx: int, vy: int) -> int:
    """A vector's walk-order key, which the plane holds: the smallest is the shortest vector, then the smallest vy, then vx."""
    return ((vx * vx + vy * vy) << 16) | ((vy + 128) << 8) | (vx + 128)


def plane(K: np.ndarray, reach: int, pass_static: bool = False, mutant=None) -> np.ndarray:
    """(H, W) uint32: fill(x, y; reach, pass_static) at every pixel, HOLE where no direction has a donor within reach."""
    K = np.ascontiguousarray(K, np.uint32)
    assert K.ndim == 2 and 1 <= reach <= REACH_MAX, (K.shape, reach)
    H, W = K.shape
    P = np.empty((H, W), np.uint32)
    _load(mutant).fill_plane(_ptr(K), W, H, int(reach), int(bool(pass_static)), _ptr(P))
    return P


def decoded(P: np.ndarray) -> np.ndarray:
    """(H, W, 2) int: the vector (x, y) a sampler takes from each word of a plane; the hole word gives (0, 0)."""
    P = np.asarray(P, np.uint32)
    v = np.stack([(P & 0xFF).astype(np.int32) - 128, ((P >> 8) & 0xFF).astype(np.int32) - 128], -1)
    v[P == HOLE] = 0
    return v


def sample(prev, curr, mv, K, P, t: float, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    out = np.empty((H, W, 4), np.uint8)
    _load().fill_mc_sample(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(_plane(K, np.uint32, (H, W))), _ptr(_plane(P, np.uint32, (H, W))),
                           W, H, float(t), int(match_sad), _ptr(out))
    return out


def sample_masked(prev, curr, mv, mask, K, P, t: float, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    prev, curr, mv = _inputs(prev, curr, mv)
    H, W = prev.shape[:2]
    out = np.empty((H, W, 4), np.uint8)
    _load().fill_ov_sample(_ptr(prev), _ptr(curr), _ptr(mv), _ptr(_plane(mask, np.uint8, (H, W))), _ptr(_plane(K, np.uint32, (H, W))),
                           _ptr(_plane(P, np.uint32, (H, W))), W, H, float(t), int(match_sad), _ptr(out))
    return out


def sample_bidirectional(prev, curr, fwd, bwd, K, P, t: float, match_sad: int = DEFAULT_MATCH_SAD, tolerance: int = 1) -> np.ndarray:
    prev, curr, fwd = _inputs(prev, curr, fwd)
    H, W = prev.shape[:2]
    out = np.empty((H, W, 4), np.uint8)
    _load().fill_bidir_sample(_ptr(prev), _ptr(curr), _ptr(fwd), _ptr(_plane(bwd, np.int8, (H, W, 2))), _ptr(_plane(K, np.uint32, (H, W))),
                              _ptr(_plane(P, np.uint32, (H, W))), W, H, float(t), int(match_sad), int(tolerance), _ptr(out))
    return out


def interpolate_compensated(prev, curr, mv, t: float, reach: int, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    K = mc_model.keys(prev, curr, mv, t, match_sad)
    return sample(prev, curr, mv, K, plane(K, reach, False), t, match_sad)


def interpolate_masked(prev, curr, mv, mask, t: float, reach: int, match_sad: int = DEFAULT_MATCH_SAD) -> np.ndarray:
    K = overlay_model.keys(prev, curr, mv, mask, t, match_sad)
    return sample_masked(prev, curr, mv, mask, K, plane(K, reach, True), t, match_sad)


def interpolate_bidirectional(prev, curr, fwd, bwd, t: float, reach: int, match_sad: int = DEFAULT_MATCH_SAD,
                              tolerance: int = 1) -> np.ndarray:
    K = bidir_model.keys(prev, curr, fwd, bwd, t, match_sad, tolerance)
    return sample_bidirectional(prev, curr, fwd, bwd, K, plane(K, reach, False), t, match_sad, tolerance)


# ---- the scene of DESIGN.md section 4.19: fast motion over a pan

SCENE_B = dict(w=160, h=96, sq=40, at=(40, 28), pan=(4, 2), shift=(48, 0))
SCENE_A = dict(w=256, h=160, sq=48, at=(100, 50), pan=(8, 4), shift=(60, 0))
BORDER = 24                                    # wrong pixels are counted further than this from the border


def fast_scene(w, h, sq, at, pan, shift, seed: int = 3, frames=(0.0, 0.5, 1.0)):
    """A noise background that pans by `pan` per pair and a noise square of side `sq`, at `at` in the first frame, that moves by
    `shift` per pair: ([the frame at each time of `frames`], the true field of the pair (0, 1)).  The true field is -pan
    everywhere and -shift on the square's place at time 1: prev(q + v) = curr(q)."""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (h + 400, w + 400, 4), dtype=np.uint8)
    tex = rng.integers(0, 256, (sq, sq, 4), dtype=np.uint8)

    def frame(tau):
        y0, x0 = 200 - round(pan[1] * tau), 200 - round(pan[0] * tau)
        f = big[y0:y0 + h, x0:x0 + w].copy()
        sx, sy = at[0] + round(shift[0] * tau), at[1] + round(shift[1] * tau)
        f[sy:sy + sq, sx:sx + sq] = tex
        return f

    field = np.zeros((h, w, 2), np.int8)
    field[...] = (-pan[0], -pan[1])
    field[at[1] + shift[1]:at[1] + shift[1] + sq, at[0] + shift[0]:at[0] + shift[0] + sq] = (-shift[0], -shift[1])
    return [frame(tau) for tau in frames], field


def wrong_pixels(frame: np.ndarray, truth: np.ndarray, border: int = BORDER) -> int:
    """Pixels of `frame` that differ from `truth` in any channel, further than `border` from the frame's border."""
    inner = (slice(border, frame.shape[0] - border), slice(border, frame.shape[1] - border))
    return int((frame[inner] != truth[inner]).any(-1).sum())
