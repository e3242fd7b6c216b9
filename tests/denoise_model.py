"""lfg_denoise_temporal restated in numpy (include/linuxfg_hip.h): the CPU model that the kernel (tests/test_gpu_denoise.py) and
the shared per-pixel header (tests/test_denoise_on_host.py) are held to byte for byte, and whose stated consequences
tests/test_denoise_model.py asserts.  Integers only, as the definition."""
import numpy as np


def _vectors(mv):
    """(vx, vy) of an (H, W, 2) field of any byte values: two's complement, dx first."""
    v = np.asarray(mv).astype(np.uint8).view(np.int8).astype(np.int64)
    return v[..., 0], v[..., 1]


def window_cost(curr, ref, mv, radius):
    """(c, n, target_inside): the window cost of `ref` displaced by `mv` at every pixel, the number of window texels inside the
    image, and whether q + v(q) lies inside it.  Window texels outside the image are skipped; ref outside reads as 0."""
    h, w = curr.shape[:2]
    c, r = curr.astype(np.int64), ref.astype(np.int64)
    vx, vy = _vectors(mv)
    ys, xs = np.mgrid[0:h, 0:w]
    cost, n = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ry, rx = ys + dy, xs + dx
            inside = (ry >= 0) & (ry < h) & (rx >= 0) & (rx < w)
            ty, tx = ry + vy, rx + vx
            t_in = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
            there = np.where(t_in[..., None], r[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)], 0)
            here = c[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)]
            cost += np.where(inside, np.abs(here - there).sum(-1), 0)
            n += inside
    ty, tx = ys + vy, xs + vx
    return cost, n, (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)


def weight(strength, L, cost, target_inside=True):
    """w = (strength * max(0, L - c)) >> 6, 0 where the vector points out of the image."""
    return np.where(target_inside, (np.int64(strength) * np.maximum(0, np.asarray(L, np.int64) - cost)) >> 6, 0)


def shares(L, w1, w2=0):
    """(a_0, a_1, a_2): a_i = floor(256 w_i / D) with D = L + w_1 + w_2, a_0 = 256 - a_1 - a_2."""
    L, w1, w2 = (np.asarray(v, np.int64) for v in (L, w1, w2))
    D = L + w1 + w2
    a1, a2 = (256 * w1) // D, (256 * w2) // D
    return 256 - a1 - a2, a1, a2


def mix(a0, a1, a2, c, r1, r2, limit):
    """One channel (or arrays of them): the rounded mix held to c +- limit."""
    c, r1, r2 = (np.asarray(v, np.int64) for v in (c, r1, r2))
    m = (a0 * c + a1 * r1 + a2 * r2 + 128) >> 8
    return np.clip(m, c - limit, c + limit)


def denoise(curr, refs, mvs, radius, tolerance, strength, limit):
    """out of lfg_denoise_temporal: curr and refs[i] (H, W, 4) uint8, mvs[i] (H, W, 2) of any byte values, one or two of each."""
    assert len(refs) == len(mvs) and 1 <= len(refs) <= 2
    h, w = curr.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    ws, theres, L = [], [], None
    for ref, mv in zip(refs, mvs):
        cost, n, t_in = window_cost(curr, ref, mv, radius)
        L = tolerance * n
        ws.append(weight(strength, L, cost, t_in))
        vx, vy = _vectors(mv)
        theres.append(ref.astype(np.int64)[np.clip(ys + vy, 0, h - 1), np.clip(xs + vx, 0, w - 1)])      # (weight 0 where clipped)
    if len(refs) == 1:
        ws.append(np.zeros((h, w), np.int64))
        theres.append(np.zeros((h, w, 4), np.int64))
    a0, a1, a2 = shares(L, ws[0], ws[1])
    return mix(a0[..., None], a1[..., None], a2[..., None], curr, theres[0], theres[1], limit).astype(np.uint8)
