"""lfg_sharpen on the CPU: a numpy restatement of the definition in include/linuxfg_hip.h, the mutants of it that the shared
inputs must tell apart, and those inputs (the CPU and the GPU tests use the same)."""
import numpy as np

MAX_STRENGTH = 64
MUTANTS = ("zero_border", "truncating_shift", "byte_clamp", "int16_product")


def sharpen(frame, strength, mutant=None):
    """frame: (h, w, channels) uint8.  out = clamp(C + ((strength * L + 32) >> 6), lo, hi) per channel, the four neighbours
    clamped to the frame.  mutant: None for the definition, or one of MUTANTS:
      zero_border       neighbours outside the frame read as 0 instead of clamped
      truncating_shift  the shift truncates toward zero instead of flooring
      byte_clamp        the limit [lo, hi] replaced by a clamp to [0, 255]
      int16_product     strength * L computed in a wrapping int16"""
    assert frame.dtype == np.uint8 and frame.ndim == 3 and 0 <= strength <= MAX_STRENGTH
    assert mutant is None or mutant in MUTANTS
    C = frame.astype(np.int32)
    p = np.pad(C, ((1, 1), (1, 1), (0, 0)), mode="constant" if mutant == "zero_border" else "edge")
    N, S, W, E = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    L = 4 * C - N - S - W - E
    lo = np.minimum.reduce([C, N, S, W, E])
    hi = np.maximum.reduce([C, N, S, W, E])
    product = strength * L
    if mutant == "int16_product":
        product = product.astype(np.int16).astype(np.int32)
    t = product + 32
    delta = np.trunc(t / 64.0).astype(np.int32) if mutant == "truncating_shift" else t >> 6
    if mutant == "byte_clamp":
        lo, hi = 0, 255
    return np.clip(C + delta, lo, hi).astype(np.uint8)


def _smoothstep(n):
    f = (np.arange(n) % 4) / 4.0
    return np.arange(n) // 4, f * f * (3.0 - 2.0 * f)


def smooth_scene(w, h, seed):
    """A random (h/4 + 3) x (w/4 + 3) lattice per channel, interpolated x4 with smoothstep weights and rounded: curved
    gradients, so that most pixels change under the sharpener and few saturate its limit."""
    lattice = np.random.default_rng(seed).integers(0, 256, (h // 4 + 3, w // 4 + 3, 4)).astype(np.float64)
    (j, ty), (i, tx) = _smoothstep(h), _smoothstep(w)
    ty, tx = ty[:, None, None], tx[None, :, None]
    top = lattice[j][:, i] * (1.0 - tx) + lattice[j][:, i + 1] * tx
    bottom = lattice[j + 1][:, i] * (1.0 - tx) + lattice[j + 1][:, i + 1] * tx
    return np.rint(top * (1.0 - ty) + bottom * ty).astype(np.uint8)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def impulses():
    """3 x 3 frames: one 255 among 0 and one 0 among 255 -- the largest |L| there is (1020)."""
    up = np.zeros((3, 3, 4), np.uint8)
    up[1, 1] = 255
    return [up, 255 - up]
