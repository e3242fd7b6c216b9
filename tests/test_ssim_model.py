"""The CPU model of lfg_frame_ssim (tests/ssim_model.py) held to account without a GPU: known answers worked out by hand, the
integer quotient against the definition in float64, every mutant of the model told apart on the scenes the GPU tests take,
lfg_frame_ssim_summarize (a pure host function) against the model's summary, and the reason the measure exists: two distortions
of equal squared error that it separates."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import ssim_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64


@pytest.fixture(scope="module")
def scenes():
    return sm.scenes(W, H)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    if not os.path.exists(capi.LIB_PATH):
        entry.build()
    return capi.load()


# ---- 1. known answers

@pytest.mark.parametrize("w,h,windows", [(8, 8, 1), (12, 8, 2), (11, 11, 1), (96, 64, 345), (9, 8, 1), (8, 12, 2)])
def test_window_count_and_identical_frames(w, h, windows):
    a = sm.scenes(w, h)["identical"][0]
    for mask in sm.MASKS:
        rec = sm.frame_ssim(a, a.copy(), mask)
        assert rec == (windows, (windows * sm.ONE,) * 4, (0,) * 64 + (windows,), sm.ONE << 33)    # worst: 2^24 + 2^24 at (0, 0)
        s = sm.summarize(rec, mask)
        assert s["all"] == 1.0 and s["ssim"] == (1.0,) * 4 and s["db"] == math.inf and s["identical"] == windows
        assert (s["worst_value"], s["worst_x"], s["worst_y"], s["below_half"]) == (1.0, 0, 0, 0)


def test_the_remainder_is_not_looked_at():
    a, b = sm.scenes(11, 11)["graded"]
    want = sm.frame_ssim(a, b)
    for x in (8, 9, 10):
        changed = b.copy()
        changed[:, x] ^= 0xFF
        changed[x] ^= 0xFF
        assert sm.frame_ssim(a, changed) == want
    changed = b.copy()
    changed[3, 7] ^= 0xFF
    assert sm.frame_ssim(a, changed) != want


def test_zero_against_255_by_hand():
    """s1 = 0, s2 = 64 * 255 = 16,320, ss = 64 * 65,025, s12 = 0: vars = 64 ss - s2^2 = 0 and covar = 0, so
    N = 416 * 235963 and D = (16320^2 + 416) * 235963; Q = floor(416 * 2^24 / 266,342,816) = floor(26.2...) = 26."""
    assert (416 << 24) // (16320 * 16320 + 416) == 26
    a, b = sm.scenes(W, H)["0-against-255"]
    rec = sm.frame_ssim(a, b)
    assert rec == (345, (345 * 26,) * 4, (345,) + (0,) * 64, (sm.ONE + 26) << 32)


def test_checkerboard_against_its_inverse_is_negative():
    """Per window s1 = s2 = 32 * 255 and s12 = 0: covar = -8160^2, the most negative there is."""
    a, b = sm.checkerboard(W, H)
    q = sm.quotients(a, b)
    assert (q == q[0, 0, 0]).all() and q[0, 0, 0] < 0
    assert q[0, 0, 0] / sm.ONE == pytest.approx(-0.99646, abs=1e-5)
    rec = sm.frame_ssim(a, b)
    assert rec[2] == (345,) + (0,) * 64 and rec[1] == (345 * int(q[0, 0, 0]),) * 4
    s = sm.summarize(rec)
    assert s["below_half"] == 345 and s["all"] < -0.99 and s["worst_value"] == q[0, 0, 0] / sm.ONE and s["db"] < 0


def test_half_and_half_windows_have_the_widest_operands():
    a, b = sm.half_and_half(W, H)
    s1, s2, ss, s12 = sm.window_sums(a, a)
    d = (s1 * s1 + s2 * s2 + 416) * (64 * ss - s1 * s1 - s2 * s2 + 235963)
    assert int(d.min()) == int(d.max()) == (2 * 8160 * 8160 + 416) * (2 * 8160 * 8160 + 235963)      # 2^53.98
    assert 2.0 ** 53.9 < int(d.max()) < 2.0 ** 54
    q = sm.quotients(a, b)
    assert (q < sm.ONE).any() and (q > sm.ONE - (1 << 12)).all()              # N is not D, and close to it


def test_range_of_the_quotient(scenes):
    for name, (a, b) in scenes.items():
        q = sm.quotients(a, b)
        assert q.min() >= -sm.ONE and q.max() <= sm.ONE, name


# ---- 2. against the definition in float64

def test_against_the_formula_in_float64(scenes):
    """Q / 2^24 is floor or ceiling of the exact N 2^24 / D, so it is within 2^-24 of N / D.  The float64 formula rounds each of
    its two products (below 2^58, not exact) and the quotient once: a relative 3 * 2^-53 and a bit, on a value of at most 1,
    call it 4 * 2^-53; the difference taken here rounds once more, 2^-53.  Every factor is an integer below 2^31, exact."""
    bound = 2.0 ** -24 + 5 * 2.0 ** -53
    for name, (a, b) in scenes.items():
        err = np.abs(sm.quotients(a, b).astype(np.float64) / sm.ONE - sm.float64_formula(a, b))
        print(f"{name}: largest |Q / 2^24 - float64| = {err.max():.3e}, bound {bound:.3e}")
        assert err.max() < bound, name


# ---- 3. the mutants

TELLS = {"narrow_n": "half-and-half", "narrow_d": "half-and-half", "round": "graded", "stride8": "graded", "remainder": None,
         "hist_all": "graded", "windows_not_added": "graded", "worst_rightmost": "identical"}


@pytest.mark.parametrize("mutant", sm.MUTANTS)
def test_mutants_differ_from_the_model(scenes, mutant):
    assert set(TELLS) == set(sm.MUTANTS)
    if mutant == "remainder":
        a, b = sm.scenes(11, 11)["graded"]                                   # (a width and height with a remainder)
    else:
        a, b = scenes[TELLS[mutant]]
    mask = 0x7
    if mutant == "windows_not_added":
        r = sm.frame_ssim(a, b, mask)
        assert sm.add(r, r, mutant) != sm.add(r, r) and sm.add(r, r)[0] == 2 * r[0]
        return
    assert sm.frame_ssim(a, b, mask, mutant) != sm.frame_ssim(a, b, mask)


def test_masks(scenes):
    a, b = scenes["graded"]
    q = sm.quotients(a, b)
    records = {mask: sm.record(q, mask) for mask in sm.MASKS}
    assert len({r[1] for r in records.values()}) == 1                        # sum does not depend on the mask
    assert len({r[2] for r in records.values()}) == len(sm.MASKS)            # hist does
    assert records[0xF][3] <= min(records[0x7][3], records[0x8][3])


# ---- 4. the host function against the model

def test_summarize_against_the_model(lib, scenes):
    for name, (a, b) in scenes.items():
        q = sm.quotients(a, b)
        for mask in sm.MASKS:
            rec = sm.record(q, mask)
            got, want = capi.summarize_ssim(rec, mask), sm.summarize(rec, mask)
            assert got == want, (name, mask, got, want)                      # the doubles too: the same operations in the same order
    r = sm.frame_ssim(*scenes["graded"])
    both = sm.add(r, sm.frame_ssim(*scenes["unrelated"]))
    assert capi.summarize_ssim(both) == sm.summarize(both) and both[0] == 690


def test_summarize_refuses(lib, scenes):
    good = sm.frame_ssim(*scenes["graded"])

    def call(rec, mask=0xF, stats=True, out=True):
        s = capi.FrameSsimStats(rec[0], (ctypes.c_int64 * 4)(*rec[1]), (ctypes.c_uint64 * 65)(*rec[2]), rec[3])
        return lib.lfg_frame_ssim_summarize(ctypes.byref(s) if stats else None, mask, ctypes.byref(capi.FrameSsimSummary()) if out else None)

    assert call(good) == 0
    short = (good[0], good[1], (good[2][0] + 1,) + good[2][1:], good[3])     # a histogram that does not sum to windows
    huge = (good[0], good[1], ((1 << 64) - 1, 1) + good[2][2:], good[3])     # ... nor by wrapping round
    empty = (0, (0,) * 4, (0,) * 65, sm.NO_WINDOW)                           # a cleared record: no windows
    assert [call(short), call(huge), call(empty), call(good, 0), call(good, 16), call(good, stats=False), call(good, out=False)] == [-1] * 7
    assert sm.summarize(short) is None and sm.summarize(empty) is None and sm.summarize(good, 0) is None
    with pytest.raises(capi.LfgError):
        capi.summarize_ssim(empty)


# ---- 5. the tiling constants the GPU tests name their sizes from

def test_binding_holds_the_kernels_tiling_constants():
    text = open(os.path.join(ROOT, "linux-fg_amd", "csrc", "frame_ssim.hip")).read()
    got = tuple(int(re.search(rf"constexpr int {name} = (\d+);", text)[1])
                for name in ("kSsimStripWindows", "kSsimSegmentRows", "kSsimWaves", "kSsimGroupsPerCu"))
    assert got == (capi.SSIM_STRIP_WINDOWS, capi.SSIM_SEGMENT_ROWS, capi.SSIM_GROUP_WAVES, capi.SSIM_GROUPS_PER_CU)
    assert ctypes.sizeof(capi.FrameSsimStats) == 568 and ctypes.sizeof(capi.FrameSsimStats) % 8 == 0


# ---- 6. why the measure is here

def test_equal_squared_error_is_told_apart():
    """One 96 x 64 synth frame under a constant offset of +8 and under +-8 of noise per byte: the same squared error within 1 %
    (64.0 and 63.96 over R, G and B; the noise clips at a few dark bytes), which PSNR cannot tell apart.  Measured on this
    model at this seed: SSIM 0.99561 under the offset and 0.97722 under the noise, a gap of 0.0184.  Held: the order, and at
    least half of that gap."""
    base = synth.make_prev(W, H, synth.BASE_SEED)
    rng = np.random.default_rng(1)
    offset = np.clip(base.astype(np.int16) + 8, 0, 255).astype(np.uint8)
    noise = np.clip(base.astype(np.int16) + rng.choice([-8, 8], size=base.shape), 0, 255).astype(np.uint8)
    mse = [float((((base.astype(np.int64) - x)[..., :3]) ** 2).mean()) for x in (offset, noise)]
    ssim = [sm.summarize(sm.frame_ssim(base, x, 0x7), 0x7)["all"] for x in (offset, noise)]
    print(f"offset +8: mse {mse[0]:.3f}, ssim {ssim[0]:.5f}; noise +-8: mse {mse[1]:.3f}, ssim {ssim[1]:.5f}")
    assert abs(mse[0] - mse[1]) <= 0.01 * mse[0]
    assert ssim[0] > ssim[1] and ssim[0] - ssim[1] >= 0.0184 / 2
