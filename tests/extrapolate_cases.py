"""Inputs that the CPU tests of the extrapolation model (tests/test_extrapolate_model.py) and the GPU tests of
lfg_extrapolate_compensated (tests/test_gpu_extrapolate.py) share, so that the two cannot drift apart: the factors, the shared
case list whose power the CPU test confirms with the model, and a plain-Python reading of a key image for that confirmation."""
from __future__ import annotations

import numpy as np

from tests import cases
from tests import extrapolate_model as ex
from tests import mc_model as mc

# 0 and 1 are the header's limits, 0.25 / 0.5 / 0.75 are exact in fp32, 1/3 is not: v / 3 is rounded before the floor.
FACTORS = [0.0, 0.25, 0.5, 1.0 / 3.0, 0.75, 1.0]
MATCH = [0, 48, 1020]


def tie_collision_foreground():
    """(prev, curr, mv): textured 16 x 8 frames for match_sad 1020, where every pixel matches.  The vectors are zero but for
    (6..8, 3), which hold (0, 2) and so move up: at a = 1 they land on row 1 and at a = 0.5 on row 2, each time on a pixel that
    also projects its own (0, 0) onto itself -- two sources collide on one destination, and the longer vector wins.  Nothing
    lands on (6..8, 3): holes.  The hole (7, 3) finds (0, 0) first in all four directions, an equal triple left and right (and
    up and down): the +x donor (9, 3) is the model's.  Its c is (7, 3) itself, matched and holding (0, 2) != (0, 0): the
    foreground.  So the output at (7, 3) is curr(9, 3); (6, 3) finds its -x neighbour at k = 1 and +x at k = 3, the same triple."""
    prev, curr = cases.textured(16, 8, 71), cases.textured(16, 8, 72)
    mv = np.zeros((8, 16, 2), np.int8)
    mv[3, 6:9] = (0, 2)
    return prev, curr, mv


def moving_square_vectors():
    """(prev, curr, mv, top-left of the square in prev): mc_model.moving_square with the oracle's full-search vectors under
    the intended semantics."""
    import oracle
    prev, curr, at = mc.moving_square()
    return prev, curr, oracle.motion(prev, curr, semantics=1).astype(np.int8), at


def shared_cases():
    """[(name, prev, curr, mv, match_sad)], every one small enough for a plain-Python walk over its key image."""
    out = [("tie, collision, foreground", *tie_collision_foreground(), 1020)]
    for kind, (w, h), seed in (("uniform", (33, 17), 3), ("piecewise", (33, 17), 4), ("random", (33, 17), 5), ("random", (7, 5), 6)):
        prev, curr, mv = cases.field(kind, w, h, seed)
        for ms in MATCH:
            out.append((f"{kind} {w}x{h} match_sad={ms}", prev, curr, mv, ms))
    prev, curr, mv, _ = moving_square_vectors()
    out.append(("moving square", prev, curr, mv, 48))
    return out


# ---- a key image read in plain Python, for the test of the cases' power (small frames only)

_DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))


def walk(K: np.ndarray, x: int, y: int):
    """[(direction index, (|v|^2, vy, vx), (nx, ny))]: each direction's first non-hole pixel within 16 of hole (x, y)."""
    H, W = K.shape
    kept = []
    for d, (sx, sy) in enumerate(_DIRS):
        for k in range(1, 17):
            nx, ny = x + sx * k, y + sy * k
            if not (0 <= nx < W and 0 <= ny < H):
                break
            key = int(K[ny, nx])
            if key == ex.HOLE:
                continue
            vx, vy = (key & 0xFF) - 128, ((key >> 8) & 0xFF) - 128
            kept.append((d, (vx * vx + vy * vy, vy, vx), (nx, ny)))
            break
    return kept


def kinds(prev, curr, mv, a: float, match_sad: int):
    """Which of the kinds of pixel that the issue names this case has at factor a, as a set of names."""
    H, W = prev.shape[:2]
    K = ex.keys(prev, curr, mv, a, match_sad)
    how = ex.branches(prev, curr, mv, a, match_sad)
    found = set()
    # collisions: more matched sources land inside the image than there are pixels with a key
    v = mv.astype(np.int32)
    ys, xs = np.mgrid[0:H, 0:W]
    sx, sy = xs + v[..., 0], ys + v[..., 1]
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    p = np.zeros_like(prev)
    p[inside] = prev[sy[inside], sx[inside]]
    matched = np.abs(curr.astype(np.int32) - p.astype(np.int32)).sum(-1) <= match_sad
    dx = xs + np.floor(np.float32(0.5) - v[..., 0].astype(np.float32) * np.float32(a)).astype(np.int32)
    dy = ys + np.floor(np.float32(0.5) - v[..., 1].astype(np.float32) * np.float32(a)).astype(np.int32)
    landed = matched & (dx >= 0) & (dx < W) & (dy >= 0) & (dy < H)
    assert len({(int(x), int(y)) for x, y in zip(dx[landed], dy[landed])}) == int((K != ex.HOLE).sum())
    if int(landed.sum()) > int((K != ex.HOLE).sum()):
        found.add("colliding projections")
    if (how == ex.NO_DONOR).any():
        found.add("holes with no donor")
    if (how == ex.DONOR_TAKEN).any():
        found.add("donor branch taken")
    for y, x in np.argwhere(K == ex.HOLE):
        x, y = int(x), int(y)
        if x in (0, W - 1) or y in (0, H - 1):
            found.add("holes at the image edge")
        kept = walk(K, x, y)
        u = (0, 0)
        if kept:
            best = min(t for _, t, _ in kept)
            if sum(1 for _, t, _ in kept if t == best) >= 2:
                found.add("equal triple from two directions")
            u = (best[2], best[1])
        _note_clamped(found, x, y, u, a, W, H)
    for y, x in np.argwhere(K != ex.HOLE):
        key = int(K[y, x])
        _note_clamped(found, int(x), int(y), ((key & 0xFF) - 128, ((key >> 8) & 0xFF) - 128), a, W, H)
    return found


def _note_clamped(found, x, y, u, a, W, H):
    """C = (x + 0.5) + u a lies outside the image: both taps of an axis are clamped to the edge, not just an idle second one."""
    cx = np.float32(x + 0.5) + np.float32(u[0]) * np.float32(a)
    cy = np.float32(y + 0.5) + np.float32(u[1]) * np.float32(a)
    if cx < 0 or cx > W or cy < 0 or cy > H:
        found.add("samples clamped outside the image")
