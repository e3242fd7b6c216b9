"""lfg_deband on the CPU: a numpy restatement of the definition in include/linuxfg_hip.h -- the random source, the draw, the
iterations, the noise and the rounding -- and the inputs that the CPU and the GPU tests share."""
import numpy as np

MAX_ITERATIONS, MAX_THRESHOLD, MAX_RADIUS, MAX_GRAIN = 4, 64, 32, 16
M32 = 0xFFFFFFFF


def h(k):
    """The random source, on uint64 arrays (or ints) holding 32-bit values."""
    k = np.asarray(k, np.uint64) & M32
    k = k ^ (k >> 16)
    k = (k * 0x7FEB352D) & M32
    k = k ^ (k >> 15)
    k = (k * 0x846CA68B) & M32
    return k ^ (k >> 16)


def draw(seed, x, y, iterations, radius):
    """(offsets (..., 8) int64: ox_1, oy_1, ... ox_4, oy_4, zeros past `iterations`; noise bytes (..., 3) int64) of the pixels
    (x, y) under `seed`; the three broadcast against each other."""
    seed, x, y = np.broadcast_arrays(np.asarray(seed, np.uint64), np.asarray(x, np.uint64), np.asarray(y, np.uint64))
    r0 = h(x ^ h(y ^ h(seed)))
    offsets = np.zeros(x.shape + (8,), np.int64)
    for i in range(1, iterations + 1):
        r, S = h(r0 + np.uint64(i)), radius * i
        offsets[..., 2 * i - 2] = (((r & 0xFFFF) * (2 * S + 1)) >> 16).astype(np.int64) - S
        offsets[..., 2 * i - 1] = (((r >> 16) * (2 * S + 1)) >> 16).astype(np.int64) - S
    r5 = h(r0 + np.uint64(5))
    noise = np.stack([((r5 >> (8 * c)) & 255).astype(np.int64) for c in range(3)], -1)
    return offsets, noise


def values(frame, iterations, threshold, radius, seed):
    """v of every pixel and colour channel after the iterations: (h, w, 3) int64, in quarters of a level."""
    H, W = frame.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    offsets, _ = draw(seed, xs, ys, iterations, radius)
    src = frame[..., :3].astype(np.int64)
    v = 4 * src
    for i in range(1, iterations + 1):
        ox, oy = offsets[..., 2 * i - 2], offsets[..., 2 * i - 1]
        s = np.zeros_like(v)
        for dx, dy in ((ox, oy), (-ox, -oy), (-oy, ox), (oy, -ox)):
            s += src[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]
        v = np.where(np.abs(s - v) <= threshold // i, s, v)
    return v


def deband(frame, iterations, threshold, radius, grain, seed):
    """frame: (h, w, 4) uint8.  The definition, byte for byte."""
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 4
    assert 1 <= iterations <= MAX_ITERATIONS and 0 <= threshold <= MAX_THRESHOLD and 1 <= radius <= MAX_RADIUS and 0 <= grain <= MAX_GRAIN
    H, W = frame.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    _, b = draw(seed, xs, ys, iterations, radius)
    n = ((b * (4 + 2 * grain)) >> 8) - grain
    out = frame.copy()
    out[..., :3] = np.clip((values(frame, iterations, threshold, radius, seed) + n) >> 2, 0, 255).astype(np.uint8)
    return out


def bound(iterations, threshold, grain):
    """The levels an output byte can lie from its input: ceil((T_1 + ... + T_I + G + 3) / 4)."""
    return -(-(sum(threshold // i for i in range(1, iterations + 1)) + grain + 3) // 4)


# ---- inputs

def ramp(w=480, h=64):
    """(the frame of round(100 + x / 24) in every colour channel, alpha 255; the unrounded ramp per column)."""
    exact = 100.0 + np.arange(w) / 24.0
    frame = np.empty((h, w, 4), np.uint8)
    frame[..., :3] = np.rint(exact).astype(np.uint8)[None, :, None]
    frame[..., 3] = 255
    return frame, exact


def banding(frame, exact, first=40, last=439, box=9):
    """The RMS distance, over columns first .. last, between the `box`-column mean of the frame's column means (over rows and
    colour channels) and the same mean of the unrounded ramp."""
    kernel = np.ones(box) / box
    got = np.convolve(frame[..., :3].astype(np.float64).mean(axis=(0, 2)), kernel, "same")
    want = np.convolve(exact, kernel, "same")
    return float(np.sqrt(np.mean((got - want)[first:last + 1] ** 2)))


def scene(w, h, seed):
    """A gradient scene plus texture plus a hard-edged box: slow ramps per channel (bands a few pixels wide and wider), a strip
    of random texture and a box of a level far from its surroundings; alpha varies per pixel."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    frame = np.empty((h, w, 4), np.uint8)
    for c, (ax, ay, base) in enumerate(((0.11, 0.05, 60.0), (0.04, 0.17, 120.0), (-0.07, 0.09, 200.0))):
        frame[..., c] = np.clip(np.rint(base + ax * xs + ay * ys), 0, 255).astype(np.uint8)
    frame[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    tex_w = max(w // 4, 1)
    frame[:, :tex_w, :3] = rng.integers(0, 256, (h, tex_w, 3), dtype=np.uint8)
    y0, y1, x0, x1 = h // 3, max(2 * h // 3, h // 3 + 1), w // 2, max(3 * w // 4, w // 2 + 1)
    frame[y0:y1, x0:x1, :3] = (250, 3, 128)
    return frame
