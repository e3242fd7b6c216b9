"""lfg_resample_light on the CPU: the definition in include/linuxfg_hip.h on top of the tables of tests/resample_model.py -- the two
light tables in Python floats, to_byte, the integer pipeline for a whole frame or for a region of interest of the output, and a
float64 evaluation of linear-light filtering to measure the integer pipeline against.  Only the live taps of a table are
gathered (the widest row's count, not the 64 columns of the table)."""
import math

import numpy as np

from tests import resample_model as rm

GAMMA, LINEAR, SIGMOID = range(3)
NAMES = {GAMMA: "gamma", LINEAR: "linear", SIGMOID: "sigmoid"}
MODES = (LINEAR, SIGMOID)
ONE = 16383
CENTRE, SLOPE = 0.75, 6.5


def srgb_to_linear(c):
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


def sigmoidize(L):
    offset = 1.0 / (1.0 + math.exp(SLOPE * CENTRE))
    scale = 1.0 / (1.0 + math.exp(SLOPE * (CENTRE - 1.0))) - offset
    return CENTRE - math.log(1.0 / (L * scale + offset) - 1.0) / SLOPE


def curve(light, c):
    """f(c) of the definition, c an encoded value in [0, 1]."""
    L = srgb_to_linear(c)
    return L if light == LINEAR else sigmoidize(L)


def tables(light):
    """(forward[256], threshold[255]) int64, and the least distance of a 16383 f(b / 255) + 0.5 from an integer."""
    if light not in MODES:
        raise ValueError(light)
    exact = [ONE * curve(light, b / 255.0) + 0.5 for b in range(256)]
    forward = np.array([math.floor(v) for v in exact], np.int64)
    threshold = (forward[:-1] + forward[1:] + 1) >> 1
    return forward, threshold


def tie_margin(light):
    """How near a table value comes to a rounding tie: the least distance of 16383 f(b / 255) from a half-integer."""
    exact = [ONE * curve(light, b / 255.0) + 0.5 for b in range(256)]
    return min(min(v - math.floor(v), math.floor(v) + 1.0 - v) for v in exact)


def to_byte(L, threshold):
    """The number of thresholds <= L."""
    return np.searchsorted(np.asarray(threshold, np.int64), np.asarray(L, np.int64), side="right")


def _live(t):
    """(index[out, K], weight[out, K]) of a table's live taps over resample_model._axis_indices, K the widest row's count."""
    first, count, q = (np.asarray(v) for v in t[:3])
    idx, live = rm._axis_indices(first, count)
    k = int(count.max())
    return idx[:, :k], np.where(live[:, :k], q[:, :k].astype(np.int64), 0)


def light_int(frame, tx, ty, forward, threshold):
    """The integer pipeline: frame (h, w, 4) uint8 through the tables tx of the width and ty of the height, which may be slices of
    a table (a region of interest of the output), the colour channels through forward and threshold, alpha as resample_int."""
    ix, wx = _live(tx)
    iy, wy = _live(ty)
    forward = np.asarray(forward, np.int64)
    src = frame.astype(np.int64)
    lit = np.concatenate([forward[src[..., :3]], src[..., 3:]], axis=-1)
    h = np.einsum("yptc,pt->ypc", lit[:, ix], wx)
    assert np.abs(h).max() < 2 ** 29
    colour, alpha = (h[..., :3] + 8192) >> 14, (h[..., 3:] + 128) >> 8
    assert colour.min() >= -8192 and colour.max() <= 24575 and alpha.min() >= -32768 and alpha.max() <= 32767
    v = np.einsum("qtpc,qt->qpc", np.concatenate([colour, alpha], axis=-1)[iy], wy)
    assert np.abs(v[..., :3]).max() < 2 ** 31 - 8192 and np.abs(v[..., 3:]).max() < 2 ** 31 - 2 ** 19
    L = np.clip((v[..., :3] + 8192) >> 14, 0, ONE)
    out = np.concatenate([to_byte(L, threshold), np.clip((v[..., 3:] + (1 << 19)) >> 20, 0, 255)], axis=-1)
    return out.astype(np.uint8)


def light(frame, ow, oh, filt, mode, tx=None, ty=None, lt=None, roi=None):
    """lfg_resample_light of `frame` to ow x oh; tx / ty default to the model's own tables and lt = (forward, threshold) to the
    model's own.  roi = (x0, y0, w, h) gives those output pixels alone, from the source rows their taps reach."""
    h, w = frame.shape[:2]
    if mode not in (GAMMA,) + MODES:
        raise ValueError(mode)
    if mode == SIGMOID and filt != rm.NEAREST and (ow < w or oh < h):
        raise ValueError("sigmoidal light with an axis that shrinks")
    tx = rm.table(filt, w, ow) if tx is None else tx
    ty = rm.table(filt, h, oh) if ty is None else ty
    if roi is not None:
        x0, y0, rw, rh = roi
        tx, ty = tuple(np.asarray(v)[x0:x0 + rw] for v in tx[:3]), tuple(np.asarray(v)[y0:y0 + rh] for v in ty[:3])
        r0, r1 = int(ty[0].min()), int((ty[0].astype(np.int64) + ty[1].astype(np.int64)).max())
        frame = frame[r0:r1]
        ty = (ty[0].astype(np.int64) - r0, ty[1], ty[2])
    if mode == GAMMA or filt == rm.NEAREST:
        return rm.resample_int(frame, tx, ty)
    forward, threshold = tables(mode) if lt is None else lt
    return light_int(frame, tx, ty, forward, threshold)


def linear_f64(frame, tx, ty):
    """Linear-light filtering in float64: the colour channels decoded exactly, filtered with the unquantised weights tx[3] and
    ty[3], clipped to [0, 1] and encoded with the analytic inverse, in code values 0 .. 255 and not rounded.  (h, w, 3)."""
    decode = np.array([srgb_to_linear(b / 255.0) for b in range(256)])
    lit = decode[frame[..., :3]]
    ix, lx = rm._axis_indices(np.asarray(tx[0]), np.asarray(tx[1]))
    iy, ly = rm._axis_indices(np.asarray(ty[0]), np.asarray(ty[1]))
    kx, ky = int(np.asarray(tx[1]).max()), int(np.asarray(ty[1]).max())
    wx, wy = np.where(lx, tx[3], 0.0)[:, :kx], np.where(ly, ty[3], 0.0)[:, :ky]
    h = np.einsum("yptc,pt->ypc", lit[:, ix[:, :kx]], wx)
    v = np.clip(np.einsum("qtpc,qt->qpc", h[iy[:, :ky]], wy), 0.0, 1.0)
    return 255.0 * np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
