"""CPU model of level matching, restated in numpy from include/linuxfg_hip.h (not from csrc/lfg_levels.hpp): lfg_frame_histogram,
lfg_levels_match, lfg_levels_apply, and the wrapper that lfg_set_level_matching puts around lfg_interpolate_frames[_multi].
Everything is integer arithmetic; the comparisons against the library are exact."""
from __future__ import annotations

import numpy as np

FORWARD, AT = 0, 1
MAX_SHIFT16 = 4080
_M64 = (1 << 64) - 1


def histogram(frame, record=None):
    """(pixels, hist 4 x 256 uint64) of an H x W x 4 uint8 frame; added to `record` (the same pair) where one is given."""
    h, w = frame.shape[:2]
    hist = np.stack([np.bincount(frame[..., c].reshape(-1), minlength=256) for c in range(4)]).astype(np.uint64)
    if record is None:
        return w * h, hist
    return record[0] + w * h, record[1] + hist


def _rank(cdf, targets):
    """For each target the smallest w with cdf[w] >= target, 255 where there is none."""
    return np.minimum(np.searchsorted(cdf, targets, side="left"), 255).astype(np.uint8)


def match(rec_from, rec_to, min_shift16):
    """lfg_levels_match as a dict: pixels, shift_sum, active, reserved, forward and inverse (3 x 256 uint8)."""
    (pa, ha), (pb, hb) = rec_from, rec_to
    ha, hb = np.asarray(ha, np.uint64), np.asarray(hb, np.uint64)
    forward, inverse = np.zeros((3, 256), np.uint8), np.zeros((3, 256), np.uint8)
    shift_sum = 0
    levels = np.arange(256)
    for c in range(3):
        ca, cb = np.cumsum(ha[c], dtype=np.uint64), np.cumsum(hb[c], dtype=np.uint64)
        forward[c] = _rank(cb, ca)
        inverse[c] = _rank(ca, cb)
        shift_sum += sum(int(n) * abs(int(f) - int(v)) for n, f, v in zip(ha[c], forward[c], levels))
    shift_sum &= _M64
    active = pa == pb and pa != 0 and (16 * shift_sum) & _M64 >= (int(min_shift16) * 3 * pa) & _M64
    if not active:
        forward[:] = inverse[:] = levels.astype(np.uint8)
    return {"pixels": int(pa), "shift_sum": int(shift_sum), "active": int(active), "reserved": 0, "forward": forward, "inverse": inverse}


def record_words(record):
    """A histogram record as the 1,025 words of struct lfg_frame_histogram_stats."""
    return np.concatenate([np.array([record[0]], np.uint64), np.asarray(record[1], np.uint64).reshape(-1)])


def map_bytes(m):
    """A map as the 1,560 bytes of struct lfg_levels_map."""
    head = np.array([m["pixels"], m["shift_sum"], m["active"] | (m["reserved"] << 32)], np.uint64).view(np.uint8)
    return np.concatenate([head, m["forward"].reshape(-1), m["inverse"].reshape(-1)])


def tq_of(factor) -> int:
    """(int)floorf(factor * 256.0f + 0.5f), in fp32."""
    return int(np.floor(np.float32(factor) * np.float32(256.0) + np.float32(0.5)))


def table(level_map, mode, factor=0.0):
    """The 3 x 256 bytes a frame's colour channels go through."""
    if mode == FORWARD:
        return level_map["forward"]
    tq = tq_of(factor)
    inv = level_map["inverse"].astype(np.int64)
    return (((256 - tq) * inv + tq * np.arange(256)[None, :] + 128) >> 8).astype(np.uint8)


def apply(frame, level_map, mode, factor=0.0):
    """lfg_levels_apply: a new frame; alpha is copied."""
    t = table(level_map, mode, factor)
    out = frame.copy()
    for c in range(3):
        out[..., c] = t[c][frame[..., c]]
    return out


def pair_map(prev, curr, min_shift16):
    return match(histogram(prev), histogram(curr), min_shift16)


def wrapper(prev, curr, min_shift16, call, factors, at_outputs=True, cut=None, newest=False):
    """lfg_interpolate_frames[_multi] with lfg_set_level_matching(min_shift16): `call(prev_seen, curr)` is the same call with
    the switch off and returns one frame per factor; it is given prev at curr's levels, and what it returns goes through
    LFG_LEVELS_AT at its factor unless `at_outputs` is False (extrapolation).  `cut(prev_seen, curr)`, where given, is the
    verdict of cut detection on what the stages saw: a cut shows the CALLER's frames (curr alone where `newest`).
    Returns (frames, map)."""
    m = pair_map(prev, curr, min_shift16)
    seen = apply(prev, m, FORWARD)
    if cut is not None and cut(seen, curr):
        return [curr if newest or np.float32(t) >= np.float32(0.5) else prev for t in factors], m
    outs = call(seen, curr)
    if at_outputs:
        outs = [apply(o, m, AT, t) for o, t in zip(outs, factors)]
    return list(outs), m
