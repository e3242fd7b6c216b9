"""CPU model of lfg_yuv_coefficients, lfg_nv12_to_rgba and lfg_rgba_to_nv12, restated in numpy from include/linuxfg_hip.h (not
from csrc/yuv_convert.hip), and the inputs that the CPU and GPU tests of the conversion share.

Planes are numpy arrays: ``y`` (H, W) uint8, ``uv`` (H/2, W/2, 2) uint8 with (Cb, Cr) last, ``rgba`` (H, W, 4) uint8.  All
arithmetic is in int32, as the header promises that everything fits; ``>>`` on numpy's signed integers is the arithmetic shift."""
from __future__ import annotations

import itertools
from fractions import Fraction

import numpy as np

BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
REPLICATE, LEFT = 0, 1
MATRICES, RANGES, SITINGS = (BT601, BT709), (LIMITED, FULL), (REPLICATE, LEFT)
MODES = list(itertools.product(MATRICES, RANGES, SITINGS))           # the 8 combinations
KR_KB = {BT601: (0.299, 0.114), BT709: (0.2126, 0.0722)}


def real_constants(matrix, rng):
    """(Kr, Kg, Kb, sy, sc, o) in double."""
    kr, kb = KR_KB[matrix]
    sy, sc, o = (255.0 / 219.0, 255.0 / 224.0, 16) if rng == LIMITED else (1.0, 1.0, 0)
    return kr, 1.0 - kr - kb, kb, sy, sc, o


def real_to_rgb(matrix, rng):
    """The five real coefficients cY, cRV, cGU, cGV, cBU in double."""
    kr, kg, kb, sy, sc, _ = real_constants(matrix, rng)
    return [sy, 2.0 * (1.0 - kr) * sc, 2.0 * kb * (1.0 - kb) / kg * sc, 2.0 * kr * (1.0 - kr) / kg * sc, 2.0 * (1.0 - kb) * sc]


def real_to_yuv(matrix, rng):
    """The nine real coefficients yR .. vB in double (every one from its own formula: no row is adjusted)."""
    kr, kg, kb, sy, sc, _ = real_constants(matrix, rng)
    return [kr / sy, kg / sy, kb / sy,
            -kr / (2.0 * (1.0 - kb)) / sc, -kg / (2.0 * (1.0 - kb)) / sc, 0.5 / sc,
            0.5 / sc, -kg / (2.0 * (1.0 - kr)) / sc, -kb / (2.0 * (1.0 - kr)) / sc]


def q14(x: float) -> int:
    """round(x * 2^14); the definition rests on no coefficient being a tie, which is asserted on the exact value of the double."""
    scaled = Fraction(x) * 16384
    assert (scaled - Fraction(1, 2)).denominator != 1, f"{x} * 2^14 is a tie"
    return int(np.floor(scaled + Fraction(1, 2)))


def coefficients(matrix, rng):
    """(to_rgb list of 5, to_yuv list of 9) as lfg_yuv_coefficients gives them."""
    kr, kg, kb, sy, sc, _ = real_constants(matrix, rng)
    to_rgb = [q14(v) for v in real_to_rgb(matrix, rng)]
    y_r, y_b = q14(kr / sy), q14(kb / sy)
    u_r, u_b = q14(-kr / (2.0 * (1.0 - kb)) / sc), q14(0.5 / sc)
    v_r, v_b = q14(0.5 / sc), q14(-kb / (2.0 * (1.0 - kr)) / sc)
    return to_rgb, [y_r, q14(1.0 / sy) - y_r - y_b, y_b, u_r, -u_r - u_b, u_b, v_r, -v_r - v_b, v_b]


def offset(rng):
    return 16 if rng == LIMITED else 0


def chroma8(c: np.ndarray, siting) -> np.ndarray:
    """One chroma plane (H/2, W/2) at every luma pixel (H, W), scaled by 8."""
    c = c.astype(np.int32)
    ch, cw = c.shape
    if siting == REPLICATE:
        return 8 * np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    h = np.empty((ch, 2 * cw), np.int32)
    h[:, 0::2] = 2 * c
    h[:, 1::2] = c + c[:, np.minimum(np.arange(cw) + 1, cw - 1)]
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[0::2] = 3 * h + h[np.maximum(np.arange(ch) - 1, 0)]
    out[1::2] = 3 * h + h[np.minimum(np.arange(ch) + 1, ch - 1)]
    return out


def nv12_to_rgba(y, uv, matrix, rng, siting) -> np.ndarray:
    (c_y, c_rv, c_gu, c_gv, c_bu), _ = coefficients(matrix, rng)
    yy = 8 * c_y * (y.astype(np.int32) - offset(rng)) + (1 << 16)
    cb, cr = chroma8(uv[..., 0], siting) - 1024, chroma8(uv[..., 1], siting) - 1024
    out = np.empty(y.shape + (4,), np.uint8)
    out[..., 0] = np.clip((yy + c_rv * cr) >> 17, 0, 255)
    out[..., 1] = np.clip((yy - c_gu * cb - c_gv * cr) >> 17, 0, 255)
    out[..., 2] = np.clip((yy + c_bu * cb) >> 17, 0, 255)
    out[..., 3] = 255
    return out


def rgba_to_nv12(rgba, matrix, rng, siting):
    """(y, uv)."""
    _, k = coefficients(matrix, rng)
    p = rgba[..., :3].astype(np.int32)
    h, w = p.shape[:2]
    y = np.clip(offset(rng) + ((k[0] * p[..., 0] + k[1] * p[..., 1] + k[2] * p[..., 2] + (1 << 13)) >> 14), 0, 255).astype(np.uint8)
    rows = p[0::2] + p[1::2]                                          # (H/2, W, 3): the luma rows 2j and 2j + 1
    if siting == REPLICATE:
        s, shift = rows[:, 0::2] + rows[:, 1::2], 16
    else:
        left = np.maximum(2 * np.arange(w // 2) - 1, 0)
        s, shift = rows[:, left] + 2 * rows[:, 0::2] + rows[:, 1::2], 17
    half = 1 << (shift - 1)
    uv = np.empty((h // 2, w // 2, 2), np.uint8)
    uv[..., 0] = np.clip(128 + ((k[3] * s[..., 0] + k[4] * s[..., 1] + k[5] * s[..., 2] + half) >> shift), 0, 255)
    uv[..., 1] = np.clip(128 + ((k[6] * s[..., 0] + k[7] * s[..., 1] + k[8] * s[..., 2] + half) >> shift), 0, 255)
    return y, uv


# ---- the float64 evaluation of the real matrices (what the integers approximate)

def real_rgb(y, cb, cr, matrix, rng):
    """(R, G, B) in double, clamped to [0, 255] but not rounded, of full-resolution Y, Cb, Cr."""
    c_y, c_rv, c_gu, c_gv, c_bu = real_to_rgb(matrix, rng)
    yy, u, v = c_y * (np.asarray(y, np.float64) - offset(rng)), np.asarray(cb, np.float64) - 128.0, np.asarray(cr, np.float64) - 128.0
    return tuple(np.clip(x, 0.0, 255.0) for x in (yy + c_rv * v, yy - c_gu * u - c_gv * v, yy + c_bu * u))


def real_yuv(r, g, b, matrix, rng):
    """(Y, Cb, Cr) in double, clamped to [0, 255] but not rounded, of one colour (for chroma: of a quad of that colour)."""
    k = real_to_yuv(matrix, rng)
    r, g, b = (np.asarray(x, np.float64) for x in (r, g, b))
    return (np.clip(offset(rng) + k[0] * r + k[1] * g + k[2] * b, 0.0, 255.0),
            np.clip(128.0 + k[3] * r + k[4] * g + k[5] * b, 0.0, 255.0),
            np.clip(128.0 + k[6] * r + k[7] * g + k[8] * b, 0.0, 255.0))


# ---- inputs the CPU and GPU tests share

def random_nv12(w, h, seed):
    """(y, uv): random bytes over the full range, with 0 and 255 forced into both planes (and into Cb and Cr each) so that
    both clamps of every channel fire."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    uv = rng.integers(0, 256, (h // 2, w // 2, 2), dtype=np.uint8)
    y[0, 0], y[-1, -1] = 0, 255
    uv[0, 0], uv[-1, -1] = (0, 255), (255, 0)
    return y, uv


def random_rgba(w, h, seed):
    """Random bytes over the full range (alpha included: it is ignored), black and white forced in."""
    rgba = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    rgba[0, 0, :3], rgba[-1, -1, :3] = 0, 255
    return rgba


def saturated_rgba(w, h, seed):
    """Two random frames whose top two rows are pure blue and pure red: every quad there is uniform and saturated, which under
    the full range is the only input whose Cb (blue) or Cr (red) reaches 128 + 128 before the clamp, under either siting."""
    blue, red = random_rgba(w, h, seed), random_rgba(w, h, seed + 1)
    blue[:2, :, :3], red[:2, :, :3] = (0, 0, 255), (255, 0, 0)
    return blue, red


def every_yuv_triple():
    """(y 4096 x 4096, uv 2048 x 2048 x 2): every (Y, Cb, Cr) exactly once under LFG_CHROMA_REPLICATE.  Quad q (row-major)
    carries the pair (q >> 14, (q >> 6) & 255) and the four lumas 4 (q & 63) + 0 .. 3."""
    q = np.arange(1 << 22, dtype=np.uint32).reshape(2048, 2048)
    uv = np.stack([(q >> 14).astype(np.uint8), ((q >> 6) & 255).astype(np.uint8)], axis=-1)
    base = ((q & 63) * 4).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = base, base + 1, base + 2, base + 3
    return y, uv


def every_rgb_triple():
    """4096 x 4096 RGBA: pixel p (row-major) is (p & 255, (p >> 8) & 255, p >> 16), every colour exactly once; alpha varies."""
    p = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([(p & 255).astype(np.uint8), ((p >> 8) & 255).astype(np.uint8), (p >> 16).astype(np.uint8),
                     ((p * 2654435761) >> 24).astype(np.uint8)], axis=-1)
