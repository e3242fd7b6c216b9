"""A float64 model of shaders/scale.comp (Lanczos-3, 6x6 taps).  TEST INFRASTRUCTURE ONLY.

Restated from the shader text, independently of the C oracle and of the library's host tables:

  * coordinates in fp32 exactly as the shader computes them (scale.comp:23-26,33,57):
      uv = (p + 0.5) / n_out,  pp = uv * n_in - 0.5,  f = pp - floor(pp),  s = floor(pp) - 2,
      tap k (0..5) is skipped when ((s + k) + 0.5) * (1 / n_in) < 0 or > 1;
  * weights in float64: Lanczos-3 at x = fp32((k - f) - 2), L(0) = 1, skipped taps 0, normalised by the sum of
    the taps kept.  Normalising per axis is exact: the shader's 2D skip rule (any(lessThan) / any(greaterThan))
    drops a whole row or column of taps, so the 2D weight sum factorises.

scale_f64() returns the UNROUNDED value V = sum_j sum_i wy_j wx_i byte in 0..255 units.  The shader samples
texture() at (s + k + 0.5) / n_in, which in fp32 is not always an exact texel centre; with the oracle's bilinear
sampler (lfg_oracle.c choice (3)) that moves its value away from V by at most subtexel_bound() LSB.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import default_threads

_f32 = np.float32


def lanczos3_f64(x: np.ndarray) -> np.ndarray:
    """3 sin(pi x) sin(pi x / 3) / (pi x)^2 in float64, 1 at x = 0."""
    x = np.asarray(x, np.float64)
    px = np.pi * x
    with np.errstate(divide="ignore", invalid="ignore"):
        v = 3.0 * np.sin(px) * np.sin(px / 3.0) / (px * px)
    return np.where(x == 0.0, 1.0, v)


def axis_taps(n_in: int, n_out: int):
    """Per output index p of one axis: (start s as int64 [n_out], weights float64 [n_out, 6], kept bool [n_out, 6],
    sub-texel offset a = min(frac(u), 1 - frac(u)) of each tap's sample position, float64 [n_out, 6])."""
    p = np.arange(n_out, dtype=np.float32)
    uv = (p + _f32(0.5)) / _f32(n_out)
    pp = uv * _f32(n_in) - _f32(0.5)
    fl = np.floor(pp)
    f = pp - fl
    s = fl - _f32(2.0)
    k = np.arange(6, dtype=np.float32)[None, :]
    ts = _f32(1.0) / _f32(n_in)
    sp = ((s[:, None] + k) + _f32(0.5)) * ts
    kept = ~((sp < _f32(0.0)) | (sp > _f32(1.0)))
    x = (k - f[:, None]) - _f32(2.0)                      # fp32, as the shader forms it
    raw = np.where(kept, lanczos3_f64(x), 0.0)
    w = raw / raw.sum(axis=1, keepdims=True)
    u = sp * _f32(n_in) - _f32(0.5)                       # where texture() puts the sample (lfg_oracle.c choice (3))
    fu = (u - np.floor(u)).astype(np.float64)
    a = np.where(kept, np.minimum(fu, 1.0 - fu), 0.0)
    return s.astype(np.int64), w, kept, a


def scale_f64(frame: np.ndarray, out_w: int, out_h: int, roi=None, band: int = 64, threads: int | None = None) -> np.ndarray:
    """The unrounded Lanczos-3 value of every output pixel in ``roi`` = (x0, y0, x1, y1) (default: the whole frame),
    float64 in 0..255 units, shape (y1 - y0, x1 - x0, 4).  Two passes of six taps (vertical, then horizontal), in
    bands of ``band`` output rows so that memory stays bounded by the band, not the frame."""
    f = np.asarray(frame)
    if f.ndim != 3 or f.shape[2] != 4 or f.dtype != np.uint8:
        raise ValueError(f"expected an (H, W, 4) uint8 frame, got {f.shape} {f.dtype}")
    h, w = f.shape[:2]
    x0, y0, x1, y1 = (0, 0, out_w, out_h) if roi is None else (int(v) for v in roi)
    if not (0 <= x0 < x1 <= out_w and 0 <= y0 < y1 <= out_h):
        raise ValueError(f"bad roi {roi} for {out_w}x{out_h}")
    sx, wx, _, _ = axis_taps(w, out_w)
    sy, wy, _, _ = axis_taps(h, out_h)
    sx, wx = sx[x0:x1], wx[x0:x1]
    # columns the ROI reads (skipped taps weigh 0: any in-range index will do for them)
    cx = np.clip(sx[:, None] + np.arange(6)[None, :], 0, w - 1)
    c_lo, c_hi = int(cx.min()), int(cx.max()) + 1
    cx -= c_lo
    out = np.empty((y1 - y0, x1 - x0, 4), np.float64)

    def rows(b0):
        b1 = min(b0 + band, y1)
        ry = np.clip(sy[b0:b1, None] + np.arange(6)[None, :], 0, h - 1)
        vert = np.zeros((b1 - b0, c_hi - c_lo, 4), np.float64)
        for j in range(6):
            vert += wy[b0:b1, j, None, None] * f[ry[:, j], c_lo:c_hi]
        acc = out[b0 - y0:b1 - y0]
        acc[...] = 0.0
        for i in range(6):
            g = np.take(vert, cx[:, i], axis=1)
            g *= wx[None, :, i, None]
            acc += g

    # numpy releases the GIL in these loops: bands run on a few threads (the oracle's cap, oracle.default_threads)
    with ThreadPoolExecutor(max_workers=threads or default_threads()) as ex:
        list(ex.map(rows, range(y0, y1, band)))
    return out


def subtexel_bound(in_wh, out_wh) -> float:
    """B in LSB: how far the shader's value can be from scale_f64()'s V, for any content, because texture() samples
    at fp32 positions a fraction a of a texel off the centre (the bilinear sampler blends in a neighbour with weight
    a, moving a texel by at most 255 a):
        B = 255 max_p(sum |wx| a_x) max_p(sum |wy|) + 255 max_p(sum |wx|) max_p(sum |wy| a_y)."""
    (wi, hi), (wo, ho) = in_wh, out_wh
    _, wx, _, ax = axis_taps(wi, wo)
    _, wy, _, ay = axis_taps(hi, ho)
    ex, ey = np.abs(wx), np.abs(wy)
    return float(255.0 * ((ex * ax).sum(1).max() * ey.sum(1).max() + ex.sum(1).max() * (ey * ay).sum(1).max()))


def near_half(v: np.ndarray, margin: float) -> np.ndarray:
    """Where clip(v, 0, 255) lies within ``margin`` of a rounding boundary k + 0.5 (the near-ties)."""
    c = np.clip(v, 0.0, 255.0)
    return np.abs(c - np.floor(c) - 0.5) <= margin


# ------------------------------------------------------------------ the shapes the GPU tests hold to the model

# The exact-2x kernel: input widths around one wave's 120 owned columns and four waves' 480 (owned-column and wave
# seams, a last wave with one lane pair), input heights from 1 (XCD bands with no strip, strips shorter than the five
# rows a strip reads first) to the 7 / 6 / 4 strip lengths.
SWEEP_2X_WIDTHS = (2, 4, 6, 8, 116, 118, 120, 122, 124, 238, 240, 242, 480, 482, 962)
SWEEP_2X_HEIGHTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 34, 35, 135, 136)


def sweep_2x_shapes():
    """48 input sizes: every width with three or four heights, every height with three widths (15 and 16 are coprime,
    so stepping through both lists together gives 48 distinct pairs)."""
    nw, nh = len(SWEEP_2X_WIDTHS), len(SWEEP_2X_HEIGHTS)
    return [(SWEEP_2X_WIDTHS[i % nw], SWEEP_2X_HEIGHTS[i % nh]) for i in range(3 * nh)]


# The generic kernel at ratios that ship, an odd input width at 2x, and the degenerate corners.
GENERIC_SHAPES = [((1280, 720), (1920, 1080)), ((2560, 1440), (3840, 2160)), ((1280, 720), (3840, 2160)),
                  ((3840, 2160), (1920, 1080)), ((1920, 1080), (3840, 2000)), ((1921, 1080), (3842, 2160)),
                  ((1, 1), (7, 5)), ((1, 64), (2, 128)), ((33, 17), (1, 1))]


def contents(w: int, h: int, seed: int, seam_rows=(), seam_cols=(118, 119, 120, 121, 238, 239, 240, 241)):
    """The frames the scale tests run, each aimed at one way a kernel goes wrong: {name: (h, w, 4) uint8}.
      noise     uniform, channels independent (a channel swap or a shifted column shows);
      checker   one-pixel 0/255 checkerboard (the largest overshoot of the filter: both saturations are hit);
      blocks    8-pixel 0/255 blocks;
      impulses  single 255 texels on 0 at the four corners, on the input columns ``seam_cols`` (the 2x kernel's wave
                seams) and on the input rows ``seam_rows`` (its strip and XCD-band seams);
      ramps     R = x ramp, G = y ramp, B = noise, A = checkerboard."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    chk = (((x + y) & 1) * 255).astype(np.uint8)
    imp = np.zeros((h, w), np.uint8)
    imp[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = 255
    for i, c in enumerate(c for c in seam_cols if c < w):
        imp[(5 * i) % h, c] = 255
        imp[(5 * i + h // 2) % h, c] = 255
    for i, r in enumerate(r for r in seam_rows if 0 <= r < h):
        imp[r, (37 * i) % w] = 255
        imp[r, (37 * i + w // 2) % w] = 255
    ramps = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1),
                      rng.integers(0, 256, (h, w)), chk], axis=-1).astype(np.uint8)
    return {
        "noise": rng.integers(0, 256, (h, w, 4), dtype=np.uint8),
        "checker": np.repeat(chk[..., None], 4, axis=-1),
        "blocks": np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)[..., None], 4, axis=-1),
        "impulses": np.repeat(imp[..., None], 4, axis=-1),
        "ramps": ramps,
    }
