"""lfg_deband's definition without a GPU: the consequences that include/linuxfg_hip.h states, held on the numpy model
(tests/deband_model.py); lfg_deband_draw -- the library's own draw, host code -- held to the model's; and what the call is
for, as a condition on a banded ramp.  CPU only."""
import re

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import deband_model as dm
from tests.host_cli import ROOT

SEEDS = (0, 1, 0xFFFFFFFF)


def texture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


# ---- the header states what the model is written from

def test_the_header_states_the_definition():
    text = re.sub(r"\s*\n \*\s*", " ", open(f"{ROOT}/include/linuxfg_hip.h").read())
    for piece in ("k ^= k >> 16;  k *= 0x7feb352d;  k ^= k >> 15;  k *= 0x846ca68b;  k ^= k >> 16", "r0 = h(x ^ h(y ^ h(seed)))", "r_j = h(r0 + j)",
                  "ox = (((r_i & 0xFFFF) (2 S + 1)) >> 16) - S", "oy = (((r_i >> 16) (2 S + 1)) >> 16) - S", "T_i = T / i",
                  "n_c = ((b_c (4 + 2 G)) >> 8) - G", "clamp((v + n_c) >> 2, 0, 255)", "1 <= I <= 4", "0 <= T <= 64", "1 <= R <= 32", "0 <= G <= 16",
                  "T = 0 with G = 0 copies the frame", "Flat areas and hard steps do not move", "Alpha never changes",
                  "ceil((sum T_i + G + 3) / 4) levels", "comes out as it went in when G = 0"):
        assert piece in text, piece
    assert (dm.MAX_ITERATIONS, dm.MAX_THRESHOLD, dm.MAX_RADIUS, dm.MAX_GRAIN) == (4, 64, 32, 16)


# ---- the consequences

@pytest.mark.parametrize("seed", SEEDS)
def test_a_flat_frame_does_not_move(seed):
    flat = np.empty((40, 50, 4), np.uint8)
    flat[...] = (17, 200, 3, 99)
    assert (dm.deband(flat, 4, 64, 32, 0, seed) == flat).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_a_hard_step_does_not_move(seed):
    step = np.full((40, 50, 4), 40, np.uint8)
    step[:, 25:] = 200
    assert (dm.deband(step, 4, 64, 32, 0, seed) == step).all()
    assert (dm.deband(step.transpose(1, 0, 2).copy(), 4, 64, 32, 0, seed) == step.transpose(1, 0, 2)).all()


def test_texture_is_left_alone():
    """Uniform random bytes at T = 4: a tap sum lands within one level of 4 v by chance only.  Under 2 % of the bytes change."""
    frame = texture(96, 64, 3)
    for seed in SEEDS:
        changed = float((dm.deband(frame, 4, 4, 16, 0, seed) != frame).mean())
        print(f"texture 96x64, T = 4, I = 4, seed {seed}: {100 * changed:.3f} % of the bytes changed")
        assert changed < 0.02


@pytest.mark.parametrize("I,R", [(1, 1), (2, 16), (4, 32)])
def test_threshold_0_without_grain_copies(I, R):
    for frame in (texture(67, 9, 5), dm.scene(65, 33, 6), dm.ramp(100, 8)[0]):
        for seed in SEEDS:
            assert (dm.deband(frame, I, 0, R, 0, seed) == frame).all()


def test_a_pixel_that_was_never_replaced_comes_out_as_it_went_in():
    frame = dm.scene(130, 40, 9)
    for I, T in ((1, 4), (4, 64)):
        v = dm.values(frame, I, T, 16, 1)
        kept = v == 4 * frame[..., :3].astype(np.int64)
        out = dm.deband(frame, I, T, 16, 0, 1)
        assert kept.any() and (~kept).any()
        assert (out[..., :3][kept] == frame[..., :3][kept]).all()


@pytest.mark.parametrize("I,T,G", [(1, 4, 0), (1, 64, 0), (4, 64, 0), (4, 64, 16), (3, 17, 5), (2, 0, 16)])
def test_the_distance_bound(I, T, G):
    """|v - 4 in| <= T_1 + ... + T_I, and every output within ceil((sum T_i + G + 3) / 4) levels of its input."""
    total = sum(T // i for i in range(1, I + 1))
    for frame in (dm.scene(130, 40, 12), dm.ramp(200, 16)[0], texture(67, 9, 13)):
        for seed in SEEDS:
            v = dm.values(frame, I, T, 32, seed)
            assert np.abs(v - 4 * frame[..., :3].astype(np.int64)).max() <= total
            out = dm.deband(frame, I, T, 32, G, seed)
            assert np.abs(out.astype(np.int64) - frame).max() <= dm.bound(I, T, G)
    assert dm.bound(4, 64, 16) == 38 and dm.bound(1, 0, 0) == 1           # (64 + 32 + 21 + 16 + 16 + 3) / 4 = 38


def test_alpha_never_changes():
    frame = dm.scene(67, 33, 21)
    assert len(np.unique(frame[..., 3])) > 100
    for I, T, G in ((1, 0, 0), (4, 64, 16), (2, 4, 3)):
        assert (dm.deband(frame, I, T, 16, G, 2)[..., 3] == frame[..., 3]).all()


def test_the_noise_range_and_mean():
    """n_c over all 256 bytes: within [-G, G + 3], both ends reached, mean 1.5 exactly."""
    b = np.arange(256)
    for G in range(dm.MAX_GRAIN + 1):
        n = ((b * (4 + 2 * G)) >> 8) - G
        assert n.min() == -G and n.max() == G + 3
        if 256 % (4 + 2 * G) == 0:                    # the levels are equally frequent where 4 + 2 G divides 256
            assert n.mean() == 1.5
        assert abs(n.mean() - 1.5) < 0.1


def test_seeds_differ_and_repeat():
    frame = dm.ramp(200, 16)[0]
    a, b = dm.deband(frame, 2, 4, 16, 3, 1), dm.deband(frame, 2, 4, 16, 3, 2)
    assert (a != b).any() and (a == dm.deband(frame, 2, 4, 16, 3, 1)).all()


# ---- lfg_deband_draw

def triples():
    """4,096 (seed, x, y): the corners of the ranges crossed with each other, then random ones."""
    ends, seeds = (0, 65535, 2 ** 31 - 1, 1, 65536), (0, 0xFFFFFFFF, 1, 0x80000000)
    rows = [(s, x, y) for s in seeds for x in ends for y in ends]
    rng = np.random.default_rng(17)
    while len(rows) < 4096:
        rows.append((int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 31))))
    return np.array(rows, np.uint64)


def test_the_library_draws_what_the_model_draws():
    rows = triples()
    assert len(rows) == 4096
    for I, R in ((1, 1), (2, 16), (3, 7), (4, 32)):
        want_offsets, want_noise = dm.draw(rows[:, 0], rows[:, 1], rows[:, 2], I, R)
        reach = np.repeat(R * np.arange(1, 5), 2)
        assert (np.abs(want_offsets) <= reach).all() and (want_offsets[:, 2 * I:] == 0).all()
        for k, (seed, x, y) in enumerate(rows.tolist()):
            offsets, noise = capi.deband_draw(seed, x, y, I, R)
            assert (offsets == want_offsets[k]).all() and (noise == want_noise[k]).all(), (seed, x, y, I, R)
    # the offsets reach both ends of the square
    offsets, _ = dm.draw(rows[:, 0], rows[:, 1], rows[:, 2], 4, 32)
    assert offsets[:, 6:].min() == -128 and offsets[:, 6:].max() == 128


def test_the_draw_refuses_what_is_out_of_range():
    import ctypes
    lib = capi.load()
    offsets, noise = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 3)()
    assert lib.lfg_deband_draw(1, 2, 3, 1, 1, offsets, noise) == 0
    for I, R in ((0, 16), (5, 16), (1, 0), (1, 33), (-1, 16), (1, -1)):
        assert lib.lfg_deband_draw(1, 2, 3, I, R, offsets, noise) == capi.ERR_INVALID, (I, R)
    assert lib.lfg_deband_draw(1, 2, 3, 1, 1, None, noise) == capi.ERR_INVALID
    assert lib.lfg_deband_draw(1, 2, 3, 1, 1, offsets, None) == capi.ERR_INVALID


# ---- what it is for

def test_a_banded_ramp_comes_out_smoother():
    """round(100 + x / 24), 480 x 64, R = 16, T = 4, G = 0: the distance between the 9-column mean of the column means and the
    unrounded ramp's, columns 40 .. 439, is at most half of the input's at I = 1 and at most a quarter at I = 4.  (As written:
    the input's 0.183; seeds 0, 1, 7 give 0.042, 0.039, 0.042 at I = 1 and 0.013, 0.014, 0.014 at I = 4.)"""
    frame, exact = dm.ramp(480, 64)
    before = dm.banding(frame, exact)
    print(f"ramp 480x64: input {before:.4f}")
    assert 0.15 < before < 0.22
    for seed in (0, 1, 7):
        one, four = dm.banding(dm.deband(frame, 1, 4, 16, 0, seed), exact), dm.banding(dm.deband(frame, 4, 4, 16, 0, seed), exact)
        print(f"ramp 480x64, seed {seed}: I = 1 {one:.4f}, I = 4 {four:.4f}")
        assert one <= before / 2
        assert four <= before / 4
