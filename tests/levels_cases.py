"""The scenes that the CPU tests of the level-matching model (tests/test_levels_model.py), the stand-alone host program
(tests/test_levels_on_host.py) and the GPU tests (tests/test_gpu_levels.py) share, so that the three cannot drift apart.

Pans are np.roll of random content: a rolled frame has exactly the histogram of the frame it came from, so a pure pan has a level
shift of 0 whatever its size (test_levels_model.py holds that).  synth.make_prev pans do not: at 64 x 48 the content that enters
shifts their histograms by about 5 levels."""
from __future__ import annotations

import numpy as np

from tests import cases

PAN = (3, -2)                                       # (dx, dy) of every rolled pan: curr(q) = base(q - PAN)
THRESHOLD = 32                                      # min_shift16 of the tests that use a threshold: 2 levels
SCENE = (200, 120)                                  # the size of the switch's scenes (cases.matrix_scene's)

# A fade as (gain in 256ths, offset): level v becomes min(255, ((v * gain + 128) >> 8) + offset) in the colour channels.
FADES = {"gain205": (205, 0), "gain230plus10": (230, 10)}


def fade(frame, gain, offset=0):
    out = frame.copy()
    v = ((frame[..., :3].astype(np.int32) * gain + 128) >> 8) + offset
    out[..., :3] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def rolled(base, dx, dy):
    return np.roll(base, (dy, dx), axis=(0, 1))


def base_of(w, h, seed, kind="textured"):
    if kind == "textured":
        return cases.textured(w, h, seed)
    from linux_fg_amd import synth
    assert kind == "noise", kind
    return synth.noise_bytes(w, h, synth.BASE_SEED + seed)


def pan(w, h, seed, kind="textured"):
    """(prev, curr): a pure pan; equal histograms."""
    base = base_of(w, h, seed, kind)
    return base, rolled(base, *PAN)


def faded_pan(w, h, seed, name="gain205", kind="textured"):
    """(prev, curr): the pan with curr faded."""
    prev, curr = pan(w, h, seed, kind)
    return prev, fade(curr, *FADES[name])


def halfway(w, h, seed, name="gain205", kind="textured"):
    """For a pan of even vector (2 * PAN): (prev, curr, the perfectly compensated half-way frame at curr's levels, the true
    half-way frame: the content half-way, the fade half-way)."""
    gain, offset = FADES[name]
    base = base_of(w, h, seed, kind)
    mid, end = rolled(base, *PAN), rolled(base, 2 * PAN[0], 2 * PAN[1])
    # the fade half-way between the identity and (gain, offset), in exact halves: ((256 + gain) * v + offset * 256) / 512
    true = mid.copy()
    v = (mid[..., :3].astype(np.int32) * (256 + gain) + 256 * offset + 256) >> 9
    true[..., :3] = np.clip(v, 0, 255).astype(np.uint8)
    return base, fade(end, gain, offset), fade(mid, gain, offset), true


def static(w, h, seed):
    base = cases.textured(w, h, seed)
    return base, base.copy()


SHUFFLED = (slice(60, 118), slice(100, 196))        # of SCENE: 23 % of its pixels


def switch_scenes():
    """name -> (prev, curr, min_shift16): what every route of the switch is run on.  In the pans the pixels of one region of curr
    are shuffled among themselves: the histograms stay equal, and no vector matches there, which leaves room for a cut threshold
    that the pair fails as well as for one that it passes (route_cases.ROOM on both sides).  A static pair matches everywhere:
    no threshold fails it."""
    w, h = SCENE
    p, c = pan(w, h, 11)
    c = c.copy()
    block = c[SHUFFLED].reshape(-1, 4)
    c[SHUFFLED] = block[np.random.default_rng(13).permutation(len(block))].reshape(c[SHUFFLED].shape)
    return {"faded": (p, fade(c, *FADES["gain205"]), THRESHOLD), "pan32": (p, c, THRESHOLD), "pan0": (p, c, 0),
            "static": (*static(w, h, 12), THRESHOLD)}


def record_pairs():
    """name -> (record A, record B) for lfg_levels_match beyond what frames give: hand-made (pixels, hist 4 x 256)."""
    def flat(level, pixels):
        h = np.zeros((4, 256), np.uint64)
        h[:, level] = pixels
        return pixels, h

    def spread(lo, hi, pixels, seed):
        rng = np.random.default_rng(seed)
        h = np.zeros((4, 256), np.uint64)
        for c in range(4):
            h[c, lo:hi] = np.bincount(rng.integers(lo, hi, pixels), minlength=256)[lo:hi]
        return pixels, h

    return {
        "single_levels": (flat(10, 4096), flat(200, 4096)),
        "disjoint": (spread(0, 60, 5000, 1), spread(180, 256, 5000, 2)),
        "empty_ends": (spread(40, 200, 6000, 3), spread(70, 180, 6000, 4)),
        "pixels_differ": (spread(0, 256, 5000, 5), spread(0, 256, 5001, 6)),
        "pixels_zero": ((0, np.zeros((4, 256), np.uint64)), (0, np.zeros((4, 256), np.uint64))),
        "from_empty": ((0, np.zeros((4, 256), np.uint64)), spread(0, 256, 100, 7)),
    }


MIN_SHIFTS = (0, 32, 4080)
FACTORS = (0.0, 1.0 / 256.0, 0.25, 0.5, 1.0 - 2.0 ** -24, 1.0)


def fade_stream(n=12, w=96, h=64, seed=21):
    """n frames that pan by PAN per frame, fade out over the middle frames and fade back in."""
    base = cases.textured(w, h, seed)
    gains = [256, 256, 256, 205, 160, 120, 120, 160, 205, 256, 256, 256]
    assert n == len(gains)
    return [fade(rolled(base, k * PAN[0], k * PAN[1]), gains[k]) for k in range(n)]
