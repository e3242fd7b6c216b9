"""lfg_upscale_edge on the CPU: a numpy restatement, in int64, of the definition in include/linuxfg_hip.h -- the positions of an
axis, the shape table, the per-texel analysis, the twelve weights of a pixel and the whole call, also on a region of interest
of the output -- and the inputs the CPU and the GPU tests share.  Nothing here calls the library."""
import numpy as np

COS = (256, 251, 237, 213, 181, 142, 98, 50, 0, -50, -98, -142, -181, -213, -237, -251)
SIN = (0, 50, 98, 142, 181, 213, 237, 251, 256, 251, 237, 213, 181, 142, 98, 50)
DIRECTIONS, STRENGTHS = 16, 33
FLAT = 4 * 65536
# the 4 x 4 texels around the bracket without their corners: (i, j) with tap (ax + i, ay + j)
TAPS = tuple((i, j) for j in range(-1, 3) for i in range(-1, 3) if not (i in (-1, 2) and j in (-1, 2)))
SENTINEL = 0x5A


def positions(n_in, n_out):
    """(base[n_out], frac[n_out]) int64 of one axis: N = (2p + 1) in - out over D = 2 out, floor and the remainder in 256ths."""
    p = np.arange(n_out, dtype=np.int64)
    N, D = (2 * p + 1) * n_in - n_out, 2 * n_out
    base = N // D
    return base, (256 * (N - base * D)) // D


def shape(k, q):
    """(A, B, C, lob, clp) of direction k and strength q, in Python integers."""
    c, s = COS[k], SIN[k]
    m = max(abs(c), abs(s))
    stretch = (65536 + m // 2) // m
    length = q * q
    sx = 256 + (((stretch - 256) * length) >> 10)
    sy = 256 - (length >> 3)
    lob = 2048 - ((1188 * length) >> 10)
    return ((sx * sx * c * c + sy * sy * s * s) >> 22, ((sx * sx - sy * sy) * c * s) >> 22, (sx * sx * s * s + sy * sy * c * c) >> 22, lob,
            (1 << 24) // lob)


def shapes():
    """The table (16, 33, 5) int64."""
    return np.array([[shape(k, q) for q in range(STRENGTHS)] for k in range(DIRECTIONS)], np.int64)


def _note(peaks, name, v):
    if peaks is not None:
        peaks[name] = max(peaks.get(name, 0), int(np.abs(v).max()))


def weights(row, fx, fy, peaks=None):
    """The twelve weights wt of TAPS, stacked in front: row = (A, B, C, lob, clp) and fx, fy, all int64 arrays that broadcast
    against each other.  `peaks`, a dict, collects the largest magnitude of every intermediate."""
    A, B, C, lob, clp = (np.asarray(v, np.int64) for v in row)
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    out = []
    for i, j in TAPS:
        ox, oy = 256 * i - fx, 256 * j - fy
        terms = (A * ((ox * ox) >> 4), 2 * B * ((ox * oy) >> 4), C * ((oy * oy) >> 4))
        total = terms[0] + terms[1] + terms[2]
        d2 = np.clip(total >> 10, 0, clp)
        p1, p2 = 1638 * d2, lob * d2
        t1, t2 = (p1 >> 12) - 4096, (p2 >> 12) - 4096
        s1, s2 = t1 * t1, t2 * t2
        pb = 25 * (s1 >> 12)
        b = (pb >> 4) - 2304
        pw = b * (s2 >> 12)
        out.append(pw >> 12)
        for name, v in (("A ox^2", terms[0]), ("2 B ox oy", terms[1]), ("C oy^2", terms[2]), ("d2 sum", total), ("1638 d2", p1), ("lob d2", p2),
                        ("t1^2", s1), ("t2^2", s2), ("25 t1^2", pb), ("b t2^2", pw)):
            _note(peaks, name, v)
    return np.stack(out)


def analysis(frame):
    """(dX, dY, mX, mY), each (h, w) int64: the luma differences of every texel against its clamped neighbours."""
    f = frame.astype(np.int64)
    L = np.pad(f[..., 0] + 2 * f[..., 1] + f[..., 2], 1, mode="edge")
    c, l, r, u, d = L[1:-1, 1:-1], L[1:-1, :-2], L[1:-1, 2:], L[:-2, 1:-1], L[2:, 1:-1]
    return r - l, d - u, np.maximum(np.abs(r - c), np.abs(c - l)), np.maximum(np.abs(d - c), np.abs(c - u))


def _level(A, M):
    return np.where(M == 0, 0, sum((4 * A >= k * M).astype(np.int64) for k in (1, 2, 3, 4)))


def select(frame, xs, ys, peaks=None):
    """(k, q) of the output pixels at positions xs = (ax, fx) and ys = (ay, fy): each (len(ay), len(ax)) int64."""
    h, w = frame.shape[:2]
    (ax, fx), (ay, fy) = xs, ys
    parts = analysis(frame)
    sums = [np.zeros((len(ay), len(ax)), np.int64) for _ in range(6)]                  # DX, DY, AX, AY, MX, MY
    for j in (0, 1):
        for i in (0, 1):
            wt = ((fy if j else 256 - fy)[:, None]) * ((fx if i else 256 - fx)[None, :])
            cy, cx = np.clip(ay + j, 0, h - 1)[:, None], np.clip(ax + i, 0, w - 1)[None, :]
            dX, dY, mX, mY = (p[cy, cx] for p in parts)
            for total, v in zip(sums, (dX, dY, np.abs(dX), np.abs(dY), mX, mY)):
                total += wt * v
    DX, DY, AX, AY, MX, MY = sums
    gx, gy = DX >> 10, DY >> 10
    best, k = np.full(DX.shape, -1, np.int64), np.zeros(DX.shape, np.int64)
    for n in range(DIRECTIONS):
        v = np.abs(gx * COS[n] + gy * SIN[n])
        _note(peaks, "projection", v)
        k = np.where(v > best, n, k)                                                   # (strictly: the smallest index wins a tie)
        best = np.maximum(best, v)
    q = _level(AX, MX) ** 2 + _level(AY, MY) ** 2
    flat = np.maximum(np.abs(DX), np.abs(DY)) < FLAT
    for name, v in (("DX", DX), ("DY", DY), ("4 AX", 4 * AX), ("4 AY", 4 * AY), ("4 MX", 4 * MX), ("4 MY", 4 * MY)):
        _note(peaks, name, v)
    return np.where(flat, 0, k), np.where(flat, 0, q)


def upscale(frame, out_w, out_h, xs=None, ys=None, table=None, roi=None, peaks=None):
    """frame (h, w, 4) uint8 -> (out_h, out_w, 4) uint8, or with roi = (x0, y0, w, h) that rectangle of it.  xs = (base, frac) of
    the width, ys of the height and the shape table default to the model's own; the GPU tests pass the library's."""
    h, w = frame.shape[:2]
    xs = positions(w, out_w) if xs is None else tuple(np.asarray(v, np.int64) for v in xs)
    ys = positions(h, out_h) if ys is None else tuple(np.asarray(v, np.int64) for v in ys)
    table = shapes() if table is None else np.asarray(table, np.int64).reshape(DIRECTIONS, STRENGTHS, 5)
    if roi is not None:
        x0, y0, rw, rh = roi
        xs, ys = tuple(v[x0:x0 + rw] for v in xs), tuple(v[y0:y0 + rh] for v in ys)
    (ax, fx), (ay, fy) = xs, ys
    k, q = select(frame, xs, ys, peaks)
    row = np.moveaxis(table[k, q], -1, 0)                                               # (5, H, W)
    wt = weights(row, fx[None, :], fy[:, None], peaks)                                  # (12, H, W)
    src = frame.astype(np.int64)
    W, S = wt.sum(0), np.zeros(k.shape + (4,), np.int64)
    for (i, j), t in zip(TAPS, wt):
        S += t[..., None] * src[np.clip(ay + j, 0, h - 1)[:, None], np.clip(ax + i, 0, w - 1)[None, :]]
    assert W.min() > 0, "a pixel's weights do not sum to a positive number"
    _note(peaks, "2 S + W", 2 * S + W[..., None])
    corners = np.stack([src[np.clip(ay + j, 0, h - 1)[:, None], np.clip(ax + i, 0, w - 1)[None, :]] for j in (0, 1) for i in (0, 1)])
    value = np.maximum(2 * S + W[..., None], 0) // (2 * W[..., None])                   # (a negative numerator ends at lo >= 0 either way)
    return np.clip(value, corners.min(0), corners.max(0)).astype(np.uint8)


def bracket(frame, out_w, out_h):
    """(lo, hi) of every output pixel: the range of its four bracket texels per channel."""
    h, w = frame.shape[:2]
    (ax, _), (ay, _) = positions(w, out_w), positions(h, out_h)
    corners = np.stack([frame[np.clip(ay + j, 0, h - 1)[:, None], np.clip(ax + i, 0, w - 1)[None, :]] for j in (0, 1) for i in (0, 1)])
    return corners.min(0), corners.max(0)


# ---- inputs

def binary_noise(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 4)) * 255).astype(np.uint8)


def random_bytes(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def diagonal_edge(w, h, lo=40, hi=200):
    """A soft edge at about 30 degrees from the vertical, alpha included."""
    y, x = np.mgrid[0:h, 0:w]
    t = np.clip((2 * x + y - (2 * w + h) // 2 + 2) * 32, 0, 128)
    return np.repeat(((lo * (128 - t) + hi * t) // 128).astype(np.uint8)[..., None], 4, -1)


def box_down(img, n):
    """The mean of n x n blocks, rounded to nearest: (h, w, c) uint8 -> (h / n, w / n, c) uint8."""
    h, w, c = img.shape
    total = img.astype(np.int64).reshape(h // n, n, w // n, n, c).sum((1, 3))
    return ((2 * total + n * n) // (2 * n * n)).astype(np.uint8)


def scene(size, seed, shapes_n=14, ss=4):
    """Bars and discs at random angles and greys over a smooth background, rendered at ss x ss samples per pixel and box-filtered:
    (size, size, 4) uint8, the rendered truth of the quality test."""
    rng = np.random.default_rng(seed)
    n = size * ss
    y, x = (np.mgrid[0:n, 0:n] + 0.5) / ss
    img = np.stack([96 + 48 * np.sin(x / size * 3 + ph) * np.cos(y / size * 2 + ph) for ph in rng.uniform(0, 6, 3)], -1)
    for _ in range(shapes_n):
        cx, cy, colour = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(0, 255, 3)
        if rng.integers(0, 2):
            inside = (x - cx) ** 2 + (y - cy) ** 2 < rng.uniform(size / 32, size / 6) ** 2
        else:
            angle, half, length = rng.uniform(0, np.pi), rng.uniform(1.0, size / 24), rng.uniform(size / 8, size / 2)
            u, v = (x - cx) * np.cos(angle) + (y - cy) * np.sin(angle), -(x - cx) * np.sin(angle) + (y - cy) * np.cos(angle)
            inside = (np.abs(v) < half) & (np.abs(u) < length)
        img[inside] = colour
    img = np.concatenate([img, np.full((n, n, 1), 255.0)], -1)
    return np.rint(img.reshape(size, ss, size, ss, 4).mean((1, 3))).astype(np.uint8)


def psnr(a, b, channels=3):
    mse = ((a[..., :channels].astype(np.float64) - b[..., :channels].astype(np.float64)) ** 2).mean()
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
