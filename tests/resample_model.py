"""lfg_resample on the CPU: a numpy restatement of the definition in include/linuxfg_hip.h -- the per-axis table in float64 from
the rational tap rule (independent of the library's builder), the integer pipeline for any table, a float64 pipeline on the
unquantised weights, the tile plan of the kernel (csrc/lfg_resample.hpp) -- and the inputs the CPU and the GPU tests share."""
import math

import numpy as np

NEAREST, BILINEAR, CATMULL_ROM, MITCHELL, LANCZOS2, LANCZOS3 = range(6)
FILTERS = (NEAREST, BILINEAR, CATMULL_ROM, MITCHELL, LANCZOS2, LANCZOS3)
NAMES = {NEAREST: "nearest", BILINEAR: "bilinear", CATMULL_ROM: "catmull-rom", MITCHELL: "mitchell", LANCZOS2: "lanczos2",
         LANCZOS3: "lanczos3"}
SUPPORT = {BILINEAR: 1, CATMULL_ROM: 2, MITCHELL: 2, LANCZOS2: 2, LANCZOS3: 3}
MAX_TAPS = 64
ONE = 16384
RATIOS = [(1, 4), (5, 11), (13, 26), (13, 17), (24, 24), (37, 12), (64, 8), (130, 13), (96, 9)]


def _cubic(x, B, C):
    x = abs(x)
    if x < 1.0:
        return ((12.0 - 9.0 * B - 6.0 * C) * x * x * x + (-18.0 + 12.0 * B + 6.0 * C) * x * x + (6.0 - 2.0 * B)) / 6.0
    if x < 2.0:
        return ((-B - 6.0 * C) * x * x * x + (6.0 * B + 30.0 * C) * x * x + (-12.0 * B - 48.0 * C) * x + (8.0 * B + 24.0 * C)) / 6.0
    return 0.0


def _lanczos(x, a):
    if x == 0.0:
        return 1.0
    if abs(x) >= a:
        return 0.0
    px = math.pi * x
    return a * math.sin(px) * math.sin(px / a) / (px * px)


def kernel(filt, x):
    """The filter at distance x (float64)."""
    if filt == BILINEAR:
        return max(0.0, 1.0 - abs(x))
    if filt == CATMULL_ROM:
        return _cubic(x, 0.0, 0.5)
    if filt == MITCHELL:
        return _cubic(x, 1.0 / 3.0, 1.0 / 3.0)
    if filt == LANCZOS2:
        return _lanczos(x, 2.0)
    if filt == LANCZOS3:
        return _lanczos(x, 3.0)
    raise ValueError(filt)


def tap_range(filt, n_in, n_out, p):
    """The integers k with |(2k+1) out - (2p+1) in| < S * 2 max(in, out): (first k, how many).  Integers only."""
    if filt == NEAREST:
        return (2 * p + 1) * n_in // (2 * n_out), 1
    lim = SUPPORT[filt] * 2 * max(n_in, n_out)
    centre = (2 * p + 1) * n_in
    # (2k+1) out > centre - lim  <=>  k > (centre - lim - out) / (2 out)
    k0 = (centre - lim - n_out) // (2 * n_out) + 1
    k1 = k0
    while abs((2 * k1 + 1) * n_out - centre) < lim:
        k1 += 1
    assert abs((2 * (k0 - 1) + 1) * n_out - centre) >= lim and k1 > k0
    return k0, k1 - k0


def max_taps(filt, n_in, n_out):
    return max(tap_range(filt, n_in, n_out, p)[1] for p in range(n_out))


def table(filt, n_in, n_out):
    """(first[out] int32, count[out] uint32, q[out, 64] int16, w[out, 64] float64): the quantised table of the definition and
    the normalised, folded weights before quantisation.  None where a row has more than MAX_TAPS taps or sum |q| > 32768."""
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.uint32)
    q = np.zeros((n_out, MAX_TAPS), np.int16)
    w = np.zeros((n_out, MAX_TAPS), np.float64)
    D = 2 * max(n_in, n_out)
    for p in range(n_out):
        k0, n = tap_range(filt, n_in, n_out, p)
        if n > MAX_TAPS:
            return None
        if filt == NEAREST:
            first[p], count[p], q[p, 0], w[p, 0] = k0, 1, ONE, 1.0
            continue
        raw = [kernel(filt, float((2 * k + 1) * n_out - (2 * p + 1) * n_in) / float(D)) for k in range(k0, k0 + n)]
        total = 0.0
        for r in raw:
            total += r
        lo, hi = min(max(k0, 0), n_in - 1), min(max(k0 + n - 1, 0), n_in - 1)
        folded = [0.0] * (hi - lo + 1)
        for j, r in enumerate(raw):
            folded[min(max(k0 + j, 0), n_in - 1) - lo] += r / total
        quant = [int(np.rint(v * ONE)) for v in folded]
        big = max(range(len(quant)), key=lambda i: (abs(quant[i]), -i))          # the first tap of largest |q|
        quant[big] += ONE - sum(quant)
        if sum(abs(v) for v in quant) > 32768:
            return None
        first[p], count[p] = lo, hi - lo + 1
        q[p, :len(quant)] = quant
        w[p, :len(folded)] = folded
    return first, count, q, w


def _axis_indices(first, count):
    idx = first[:, None].astype(np.int64) + np.arange(MAX_TAPS)[None, :]
    live = np.arange(MAX_TAPS)[None, :] < count[:, None].astype(np.int64)
    return np.where(live, idx, first[:, None].astype(np.int64)), live


def resample_int(frame, tx, ty):
    """The integer pipeline: frame (h, w, 4) uint8 through the tables tx = (first, count, q) of the width and ty of the height."""
    fx, cx, qx = tx[:3]
    fy, cy, qy = ty[:3]
    ix, lx = _axis_indices(np.asarray(fx), np.asarray(cx))
    iy, ly = _axis_indices(np.asarray(fy), np.asarray(cy))
    wx = np.where(lx, np.asarray(qx, np.int64), 0)
    wy = np.where(ly, np.asarray(qy, np.int64), 0)
    src = frame.astype(np.int64)
    h = np.einsum("yptc,pt->ypc", src[:, ix], wx)                       # (in_h, out_w, 4), exact
    assert np.abs(h).max() < 2 ** 31
    h = (h + 128) >> 8
    assert h.min() >= -32768 and h.max() <= 32767
    v = np.einsum("qtpc,qt->qpc", h[iy], wy)
    assert np.abs(v).max() < 2 ** 31 - 2 ** 19
    return np.clip((v + (1 << 19)) >> 20, 0, 255).astype(np.uint8)


def resample_f64(frame, tx, ty):
    """The float64 separable evaluation with the unquantised weights tx[3], ty[3]: the unrounded, unclipped values."""
    ix, lx = _axis_indices(np.asarray(tx[0]), np.asarray(tx[1]))
    iy, ly = _axis_indices(np.asarray(ty[0]), np.asarray(ty[1]))
    wx, wy = np.where(lx, tx[3], 0.0), np.where(ly, ty[3], 0.0)
    h = np.einsum("yptc,pt->ypc", frame.astype(np.float64)[:, ix], wx)
    return np.einsum("qtpc,qt->qpc", h[iy], wy)


def resample(frame, out_w, out_h, filt):
    """frame through the model's own tables."""
    h, w = frame.shape[:2]
    return resample_int(frame, table(filt, w, out_w), table(filt, h, out_h))


# ---- the kernel's tile plan (csrc/lfg_resample.hpp: resample_plan)

TILE_COLUMNS = 64
LDS_ROWS = 64


def plan_rows(first, count):
    """(T, span): the output rows per tile -- the largest of 16, 8, 4, 2, 1 at which the source rows of every tile,
    first[q0] .. first[q1 - 1] + count[q1 - 1], hold each of its rows' taps and number at most LDS_ROWS -- and the largest
    number of source rows a tile then needs."""
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    n = len(first)
    for T in (16, 8, 4, 2, 1):
        span, ok = 0, True
        for q0 in range(0, n, T):
            q1 = min(q0 + T, n)
            lo, hi = first[q0], first[q1 - 1] + count[q1 - 1]
            ok = ok and hi - lo <= LDS_ROWS and (first[q0:q1] >= lo).all() and (first[q0:q1] + count[q0:q1] <= hi).all()
            span = max(span, int(hi - lo))
        if ok:
            return T, span
    raise AssertionError("a single row always fits")


# ---- inputs

def stripes(w, h):
    """One-pixel vertical stripes 0, 255, 0, 255, ... in every channel."""
    f = np.zeros((h, w, 4), np.uint8)
    f[:, 1::2] = 255
    return f


def binary_noise(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 4)) * 255).astype(np.uint8)


# ---- the cases the CPU run of the kernel (tests/test_resample_on_host.py) and the GPU test share

# (in w, in h, out w, out h): the smallest input; a small upscale; exact 2x; an inexact upscale; identity; 3 : 1 down;
# 48 taps; 64 taps, the limit; one column over a tile and exactly one tile wide; three tiles wide and more than T rows
SHAPES = [(1, 1, 4, 3), (5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (24, 16, 24, 16), (37, 19, 12, 6), (64, 9, 8, 3),
          (96, 8, 9, 2), (33, 5, 65, 9), (70, 6, 64, 4), (67, 9, 130, 20)]
# 8 x h -> 8 x 20: under Lanczos-3 a tile of 8 / 4 / 2 output rows needs more than LDS_ROWS source rows at 5.5 : 1 / 8 : 1 /
# 10 : 1, which forces T = 4 / 2 / 1.  (A source of 64 rows, as in 8 x 64 -> 8 x h, fits whole: T = 16 at every ratio.)
SMALL_T = {4: (8, 110, 8, 20), 2: (8, 160, 8, 20), 1: (8, 200, 8, 20)}
SENTINEL = 0x5A


def up16(n):
    return (n + 15) // 16 * 16


def layouts(w):
    """name -> (pitch, lead) of a frame w pixels wide.  tight: as lfg_frame_create lays a frame out; dword: a pitch 4 bytes
    longer behind a 4-byte lead, nothing 16-byte aligned; aligned: base and pitch multiples of 16 with padding."""
    return {"tight": (w * 4, 0), "dword": (w * 4 + 4, 4), "aligned": (up16(w * 4) + 16, 32)}
