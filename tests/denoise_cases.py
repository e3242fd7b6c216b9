"""The cases that the denoiser's suites share: tests/test_denoise_model.py (the model's stated consequences),
tests/test_gpu_denoise.py (lfg_denoise_temporal against the model) and tools/denoise_bench.py (the noisy streams).  Everything
is generated from a seed."""
import numpy as np

from linux_fg_amd import synth

# 1 x 1, 3 x 2; 64 x 4 is one workgroup exactly, 65 x 5 one past it in both axes, 130 x 9 three by three of them
SHAPES = [(1, 1), (3, 2), (64, 4), (65, 5), (130, 9)]
RADII = (0, 1, 2)
COUNTS = (1, 2)
# (tolerance, strength, limit) at the ends of their ranges
EXTREMES = [(t, s, l) for t in (1, 1020) for s in (1, 256) for l in (1, 255)]


def scene(w, h, seed):
    """A smooth pattern with a few hard edges, all four channels different, bytes in 16 .. 239."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 4), np.uint8)
    for c in range(4):
        fx, fy, p = rng.uniform(0.05, 0.4, 3)
        v = 128 + 70 * np.sin(fx * x + p) * np.cos(fy * y - p) + 30 * ((x // 7 + y // 5 + c) % 2)
        out[..., c] = np.clip(np.rint(v), 16, 239)
    return out


def random_frame(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def noisy(clean, amplitude, seed):
    """`clean` plus independent uniform noise of -amplitude .. amplitude levels on R, G and B, clipped to bytes."""
    n = np.random.default_rng(seed).integers(-amplitude, amplitude + 1, clean.shape)
    n[..., 3] = 0
    return np.clip(clean.astype(np.int64) + n, 0, 255).astype(np.uint8)


def mse(a, b):
    return float(((a.astype(np.int64) - b.astype(np.int64)) ** 2).mean())


def constant_field(w, h, vx, vy):
    mv = np.empty((h, w, 2), np.int8)
    mv[..., 0], mv[..., 1] = vx, vy
    return mv


def random_field(w, h, seed):
    """Every byte value, -128 included."""
    return np.random.default_rng(seed).integers(-128, 128, (h, w, 2), dtype=np.int8)


def small_field(w, h, seed, reach=2):
    return np.random.default_rng(seed).integers(-reach, reach + 1, (h, w, 2), dtype=np.int8)


def outward_field(w, h):
    """Zero inside; every border pixel points out of the image, across its nearest edge (a corner across both)."""
    mv = np.zeros((h, w, 2), np.int8)
    mv[:, 0, 0], mv[:, -1, 0] = -1, 1
    mv[0, :, 1], mv[-1, :, 1] = -1, 1
    if w == 1:
        mv[:, 0, 0] = -1
    if h == 1:
        mv[0, :, 1] = 1
    return mv


def fields(w, h, seed):
    return {"constant": constant_field(w, h, 2, -1), "random": random_field(w, h, seed), "outward": outward_field(w, h)}


def pan_stream(w, h, frames, shift=(3, -2), seed=synth.BASE_SEED):
    """`frames` clean frames of one textured plane seen through a window that moves, so that frame k + 1 at q is frame k at
    q - shift everywhere (no exposed strip): lfg_motion(frame k, frame k + 1) should give -shift."""
    sx, sy = shift
    pad_x, pad_y = abs(sx) * (frames - 1), abs(sy) * (frames - 1)
    plane = synth.make_prev(w + pad_x, h + pad_y, seed)
    out = []
    for k in range(frames):
        x0 = pad_x - sx * k if sx > 0 else -sx * k
        y0 = pad_y - sy * k if sy > 0 else -sy * k
        out.append(np.ascontiguousarray(plane[y0:y0 + h, x0:x0 + w]))
    return out
