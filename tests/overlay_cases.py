"""Inputs that the CPU tests of the overlay model (tests/test_overlay_model.py) and the GPU tests of
lfg_interpolate_compensated_masked (tests/test_gpu_overlay.py) share: the overlay scenes of DESIGN.md section 4.13, the flat
moving square, and the hand-made cases, each stated through the public inputs alone."""
from __future__ import annotations

import numpy as np

from linux_fg_amd import synth
from tests import cases

W, H = 200, 120
SEED = synth.BASE_SEED + 5
WHITE = (255, 255, 255, 255)

# ---- the overlay scenes: a panned background under an overlay that holds the same bytes in prev, curr and the truth

OVERLAYS = ("glyphs", "cross", "panel")
PANS = ((6, -4), (12, 8))
SCENES = [(o, p) for o in OVERLAYS for p in PANS]


def overlay(kind: str):
    """(on, bytes): the (H, W) bool image of the overlay's pixels and the (H, W, 4) image that holds their bytes."""
    on = np.zeros((H, W), bool)
    px = np.zeros((H, W, 4), np.uint8)
    if kind == "glyphs":                     # eight E-like glyphs, a 1 px bar and a 2 px bar: 402 pixels
        for k in range(8):
            x, y = 20 + 10 * k, 12
            on[y:y + 9, x] = True
            for r in (y, y + 4, y + 8):
                on[r, x:x + 6] = True
        on[100, 10:190] = True
        on[96:112, 150:152] = True
        px[on] = WHITE
    elif kind == "cross":                    # a crosshair: 41 pixels
        on[60, 90:111] = True
        on[50:71, 100] = True
        px[on] = WHITE
    else:                                    # a panel of noise: 1,200 pixels
        assert kind == "panel", kind
        on[90:110, 20:80] = True
        px[90:110, 20:80] = np.random.default_rng(3).integers(0, 256, (20, 60, 4), dtype=np.uint8)
    return on, px


def scene(kind: str, pan, t: float = 0.5):
    """(prev, curr, truth at time t, on): pan * t must be whole pixels."""
    bg = synth.make_prev(W, H, SEED)
    at = (pan[0] * t, pan[1] * t)
    assert at[0] == int(at[0]) and at[1] == int(at[1]), (pan, t)
    frames = [bg.copy(), synth.translate(bg, pan, SEED), synth.translate(bg, (int(at[0]), int(at[1])), SEED)]
    on, px = overlay(kind)
    for f in frames:
        f[on] = px[on]
    return frames[0], frames[1], frames[2], on


def near(on: np.ndarray, reach: int = 8) -> np.ndarray:
    """The pixels within `reach` px (Chebyshev) of the overlay but not on it."""
    h, w = on.shape
    out = np.zeros_like(on)
    ys, xs = np.nonzero(on)
    for y, x in zip(ys, xs):
        out[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = True
    return out & ~on


def wrong(got: np.ndarray, truth: np.ndarray) -> np.ndarray:
    """(H, W) bool: R, G or B differs from the truth."""
    return (got[..., :3] != truth[..., :3]).any(-1)


def interior(shape, margin: int = 16) -> np.ndarray:
    """The pixels more than `margin` px from the image edge."""
    m = np.zeros(shape, bool)
    m[margin:-margin, margin:-margin] = True
    return m


def flat_moving_square():
    """(prev, curr, truth at t = 0.5): a flat-coloured 32 px square moving by (10, 6) over a pan of (4, -2).  The overlap of
    the square with itself is static by lfg_static_mask's test, and is no overlay."""
    bg = synth.make_prev(W, H, SEED)
    frames = [bg.copy(), synth.translate(bg, (4, -2), SEED), synth.translate(bg, (2, -1), SEED)]
    for f, (dx, dy) in zip(frames, ((0, 0), (10, 6), (5, 3))):
        f[40 + dy:72 + dy, 80 + dx:112 + dx] = (200, 60, 30, 255)
    return tuple(frames)


def bare_pan(pan=(6, -4)):
    bg = synth.make_prev(W, H, SEED)
    return bg, synth.translate(bg, pan, SEED)


# ---- the hand-made cases.  Each is (prev, curr, mv, mask, match_sad): textured frames and match_sad 1020, so that every pixel
# passes the match gate and a generated frame shows which vector and which rule each pixel was sampled with.  At t = 0.5 a
# vector v projects by floor(v * 0.5 + 0.5).

def _textured(w, h, seed):
    return cases.textured(w, h, seed), cases.textured(w, h, seed + 1), np.zeros((h, w, 2), np.int8), np.zeros((h, w), np.uint8)


def static_under_collision(value: int = 255):
    """8 x 8: (4, 4) is static, and the longest vector of the frame, (6, 4)'s (-4, 0), lands on it: K(4, 4) stays 0 and the
    output there is the mix of the two texels.  (4, 4) also projects its own vector (2, 0), which wins (5, 4) over that pixel's
    (0, 0); there the fetch rule finds c = (4, 4) static and takes prev's sample alone.  `value`: the mask byte."""
    prev, curr, mv, mask = _textured(8, 8, 71)
    mv[4, 6] = (-4, 0)
    mv[4, 4] = (2, 0)
    mask[4, 4] = value
    return prev, curr, mv, mask, 1020


def walk_past_static_run():
    """12 x 1, so that the walk has two directions.  Pixels 0 .. 5 are holes (their vectors leave the image), 6 and 7 static,
    and 8 holds (-4, 0), which came from pixel 10: hole 5's only non-hole within reach lies behind the static run, and its
    fill vector is (-4, 0) -- (0, 0) if the walk stopped at pixel 6."""
    prev, curr, mv, mask = _textured(12, 1, 73)
    mv[0, 0:6] = (0, -4)
    mv[0, 8] = (0, -4)
    mv[0, 10] = (-4, 0)
    mask[0, 6:8] = 255
    return prev, curr, mv, mask, 1020


def rule_on_projected_pixels():
    """12 x 8.  Row 2: (5, 2)'s vector (2, 0) lands on (6, 2), where P.x = 7.5 and C.x = 5.5; (7, 2) is static, so p is and c
    is not: curr's sample alone.  Row 5 likewise with (5, 5) static: c is and p is not: prev's sample alone.  Rounded to
    nearest the positions would be 8 and 6, neither static."""
    prev, curr, mv, mask = _textured(12, 8, 75)
    mv[2, 5] = (2, 0)
    mv[5, 5] = (2, 0)
    mask[2, 7] = 255
    mask[5, 5] = 255
    return prev, curr, mv, mask, 1020


def rule_on_a_hole(static_p: bool):
    """16 x 1.  Pixels 0 .. 8 are holes, and hole 8 takes its fill vector u from pixel 9.
    static_p: 9 holds (-2, 0) (from pixel 10), so P.x = 7.5 and C.x = 9.5, and pixel 7 is static: curr's sample alone,
    although mv(9) != u would say covered (prev's alone) if the hole's own test came first.
    Otherwise 9 holds (-4, 0) (from pixel 11), so P.x = 6.5 and C.x = 10.5, and pixel 10 is static: prev's sample alone."""
    prev, curr, mv, mask = _textured(16, 1, 77 if static_p else 79)
    mv[0, 0:10] = (0, -4)
    if static_p:
        mv[0, 10] = (-2, 0)                  # -> 9
        mask[0, 7] = 255
    else:
        mv[0, 11] = (-4, 0)                  # -> 9: u = (-4, 0), P.x = 6.5, C.x = 10.5
        mask[0, 10] = 255
    return prev, curr, mv, mask, 1020


def region_of_interest():
    """(prev, curr, mv, mask, match_sad, (x, y, w, h)) of 96 x 64 frames: the call sees the ROI alone, as views into the four
    arrays, and must give what the model gives on the crops."""
    prev, curr, mv = cases.field("random", 96, 64, 81)
    mask = (np.random.default_rng(82).random((64, 96)) < 0.3).astype(np.uint8) * 255
    return prev, curr, mv, mask, 1020, (20, 12, 51, 37)


def random_masked(w: int, h: int, seed: int):
    """cases.field("random") with a 30 % random mask whose static bytes take every non-zero value."""
    prev, curr, mv = cases.field("random", w, h, seed)
    rng = np.random.default_rng(seed + 1000)
    mask = np.where(rng.random((h, w)) < 0.3, rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
    return prev, curr, mv, mask, 1020


def hand_made():
    """{name: (prev, curr, mv, mask, match_sad)}: what test_overlay_model.py tells the mutants apart with and
    test_gpu_overlay.py runs on the GPU."""
    return {
        "static under collision": static_under_collision(),
        "mask byte 1": static_under_collision(1),
        "mask byte 128": static_under_collision(128),
        "walk past a static run": walk_past_static_run(),
        "rule on projected pixels": rule_on_projected_pixels(),
        "rule on a hole, p static": rule_on_a_hole(True),
        "rule on a hole, c static": rule_on_a_hole(False),
    }
