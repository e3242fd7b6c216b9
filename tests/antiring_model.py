"""lfg_resample_antiring on the CPU: the definition in include/linuxfg_hip.h on top of the tables of tests/resample_model.py --
the brackets in plain Python integers, and the integer pipeline with each qualifying pass mixed towards the range of its
bracket, for a whole frame or for a region of interest of the output.  Only the live taps of a table are gathered (the widest
row's count, 6 for an upscale under Lanczos-3, not the 64 columns of the table)."""
import numpy as np

from tests import resample_model as rm

MAX_STRENGTH = 64
# what the anti-ringing tests add to resample_model.SHAPES: one pass qualifies (the other axis shrinks), and resample_model.SMALL_T's
# downscales with the width doubled -- the horizontal pass qualifies while the vertical table forces T = 4 / 2 / 1.  (A growing
# height cannot force a small T: an upscale has at most 6 taps per row, and 16 output rows need far fewer than 64 source rows.)
HORIZONTAL_ONLY, VERTICAL_ONLY = (13, 26, 26, 13), (26, 13, 13, 26)
SMALL_T_UP = {rows: (w, h, 2 * ow, oh) for rows, (w, h, ow, oh) in rm.SMALL_T.items()}


def brackets(n_in, n_out):
    """(a[n_out], b[n_out]): floor and ceiling of the output centre ((2p + 1) in - out) / (2 out) in texels, clamped to the axis."""
    lo, hi = [], []
    for p in range(n_out):
        N, D = (2 * p + 1) * n_in - n_out, 2 * n_out
        lo.append(min(max(N // D, 0), n_in - 1))
        hi.append(min(max(-((-N) // D), 0), n_in - 1))
    return np.array(lo, np.int64), np.array(hi, np.int64)


def strengths(filt, w, h, ow, oh, strength):
    """(sx, sy): the strength each pass runs with -- `strength` where it is anti-ringed, else 0."""
    rings = strength > 0 and filt != rm.NEAREST
    return (strength if rings and ow > w else 0), (strength if rings and oh > h else 0)


def _live(t):
    """(index[out, K], weight[out, K]) of a table's live taps, K the widest row's count; dead taps read the first one with weight 0."""
    first, count, q = (np.asarray(v) for v in t[:3])
    k = int(count.max())
    live = np.arange(k)[None, :] < count[:, None].astype(np.int64)
    return np.where(live, first[:, None].astype(np.int64) + np.arange(k)[None, :], first[:, None].astype(np.int64)), np.where(live, q[:, :k].astype(np.int64), 0)


def _mix(s, x, y, strength):
    """s + floor((clamp(s, 16384 min(x, y), 16384 max(x, y)) - s) strength / 64) in int64, and where the clamp bound."""
    lo, hi = rm.ONE * np.minimum(x, y), rm.ONE * np.maximum(x, y)
    d = np.clip(s, lo, hi) - s
    assert np.abs(d).max(initial=0) < 2 ** 31
    return s + ((d * strength) >> 6), d != 0


def antiring_int(frame, tx, ty, sx, sy, bx=None, by=None, bound=False):
    """frame (h, w, 4) uint8 through the tables tx of the width and ty of the height, which may be slices of a table (a region of
    interest of the output), the horizontal pass at strength sx with the brackets bx = (a, b) and the vertical one at sy with by.
    With bound=True also the (out h, out w, 4) mask of the bytes at which a clamp bound: the vertical one, or the horizontal one
    at any h' the byte's taps read."""
    ix, wx = _live(tx)
    iy, wy = _live(ty)
    src = frame.astype(np.int64)
    h = np.einsum("yptc,pt->ypc", src[:, ix], wx)
    assert np.abs(h).max() < 2 ** 31
    bound_h = np.zeros(h.shape, bool)
    if sx:
        h, bound_h = _mix(h, src[:, np.asarray(bx[0])], src[:, np.asarray(bx[1])], sx)
    h = (h + 128) >> 8
    assert h.min() >= -32768 and h.max() <= 32767
    v = np.einsum("qtpc,qt->qpc", h[iy], wy)
    assert np.abs(v).max() < 2 ** 31 - 2 ** 19
    bound_v = np.zeros(v.shape, bool)
    if sy:
        v, bound_v = _mix(v, h[np.asarray(by[0])], h[np.asarray(by[1])], sy)
    out = np.clip((v + (1 << 19)) >> 20, 0, 255).astype(np.uint8)
    if not bound:
        return out
    return out, bound_v | bound_h[iy].any(1)                           # (a dead tap's index is the first tap's: live)


def antiring(frame, ow, oh, filt, strength, tx=None, ty=None, bound=False, roi=None):
    """lfg_resample_antiring of `frame` to ow x oh; tx / ty default to the model's own tables.  roi = (x0, y0, w, h) gives those
    output pixels alone, from the source rows their taps reach."""
    h, w = frame.shape[:2]
    tx = rm.table(filt, w, ow) if tx is None else tx
    ty = rm.table(filt, h, oh) if ty is None else ty
    sx, sy = strengths(filt, w, h, ow, oh, strength)
    bx, by = brackets(w, ow) if sx else None, brackets(h, oh) if sy else None
    if roi is not None:
        x0, y0, rw, rh = roi
        tx, ty = tuple(np.asarray(v)[x0:x0 + rw] for v in tx[:3]), tuple(np.asarray(v)[y0:y0 + rh] for v in ty[:3])
        bx = None if bx is None else tuple(v[x0:x0 + rw] for v in bx)
        by = None if by is None else tuple(v[y0:y0 + rh] for v in by)
        r0, r1 = int(ty[0].min()), int((ty[0].astype(np.int64) + ty[1].astype(np.int64)).max())
        frame = frame[r0:r1]
        ty = (ty[0].astype(np.int64) - r0, ty[1], ty[2])
        by = None if by is None else tuple(v - r0 for v in by)
    return antiring_int(frame, tx, ty, sx, sy, bx, by, bound)


def step(w, h, left, right):
    """A hard vertical edge in the middle of the frame, every channel alike."""
    f = np.full((h, w, 4), left, np.uint8)
    f[:, w // 2:] = right
    return f
