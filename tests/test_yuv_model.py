"""lfg_yuv_coefficients (a pure host function: no GPU) against the CPU model's derivation (tests/yuv_model.py), and the model
itself: exact row sums, the known answers of the standards, +-1 LSB against a float64 evaluation of the real matrices for every
input in both directions, the two sitings on constant chroma, the clamped edges at 2 x 2.  CPU only."""
import os

import numpy as np
import pytest

from tests import yuv_model as ym

MATRIX_RANGE = [(m, r) for m in ym.MATRICES for r in ym.RANGES]
NAMES = {(ym.BT601, ym.LIMITED): "601-limited", (ym.BT601, ym.FULL): "601-full", (ym.BT709, ym.LIMITED): "709-limited",
         (ym.BT709, ym.FULL): "709-full"}
mr = pytest.mark.parametrize("matrix,rng", MATRIX_RANGE, ids=[NAMES[k] for k in MATRIX_RANGE])


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as entry
    from linux_fg_amd import capi as c
    if not os.path.exists(c.LIB_PATH):
        entry.build()
    return c


def grey_nv12(value, w=2, h=2):
    return np.full((h, w), value, np.uint8), np.full((h // 2, w // 2, 2), 128, np.uint8)


def solid(r, g, b, w=2, h=2):
    return np.broadcast_to(np.array([r, g, b, 7], np.uint8), (h, w, 4)).copy()


# ---- 1. the library's coefficients are the model's

@mr
def test_library_coefficients_equal_the_derivation(capi, matrix, rng):
    to_rgb, to_yuv = capi.yuv_coefficients(matrix, rng)
    want_rgb, want_yuv = ym.coefficients(matrix, rng)
    assert list(to_rgb) == want_rgb and list(to_yuv) == want_yuv


def test_library_coefficients_refuse_bad_arguments(capi):
    import ctypes
    lib = capi.load()
    a, b = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 9)()
    for matrix, rng in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        assert lib.lfg_yuv_coefficients(matrix, rng, a, b) == -1
    assert lib.lfg_yuv_coefficients(0, 0, None, b) == -1 and lib.lfg_yuv_coefficients(0, 0, a, None) == -1
    assert lib.lfg_yuv_coefficients(1, 1, a, b) == 0


# ---- 2. the coefficients: exact row sums, each within half a unit of 2^-14 of its real value (the three adjusted ones: 1.5)

@mr
def test_rows_sum_exactly(matrix, rng):
    _, k = ym.coefficients(matrix, rng)
    sy = ym.real_constants(matrix, rng)[3]
    assert k[0] + k[1] + k[2] == ym.q14(1.0 / sy)
    assert k[3] + k[4] + k[5] == 0 and k[6] + k[7] + k[8] == 0
    if rng == ym.FULL:
        assert k[0] + k[1] + k[2] == 1 << 14 and k[5] == k[6] == 1 << 13


@mr
def test_coefficients_are_near_their_real_values(matrix, rng):
    to_rgb, to_yuv = ym.coefficients(matrix, rng)
    for got, real in zip(to_rgb, ym.real_to_rgb(matrix, rng)):
        assert abs(got - real * 16384.0) <= 0.5
    for i, (got, real) in enumerate(zip(to_yuv, ym.real_to_yuv(matrix, rng))):
        assert abs(got - real * 16384.0) <= (1.5 if i in (1, 4, 7) else 0.5), i


# ---- 3. known answers

@pytest.mark.parametrize("siting", ym.SITINGS)
@mr
def test_every_grey(matrix, rng, siting):
    """Black, white and every grey: Cb = Cr = 128 and, under the full range, R = G = B = Y both ways."""
    v = np.arange(256, dtype=np.uint8)
    grey = np.repeat(np.repeat(v.reshape(16, 16), 2, axis=0), 2, axis=1)                 # 32 x 32: one grey per quad
    rgba = np.stack([grey, grey, grey, 255 - grey], axis=-1)
    y, uv = ym.rgba_to_nv12(rgba, matrix, rng, ym.REPLICATE)                             # (LEFT mixes neighbouring greys: below)
    assert (uv == 128).all()
    for g in (0, 1, 127, 128, 254, 255):
        yy, cc = ym.rgba_to_nv12(solid(g, g, g, 6, 4), matrix, rng, siting)
        assert (cc == 128).all() and (yy == yy[0, 0]).all()
    if rng == ym.FULL:
        assert (y == grey).all()
        back = ym.nv12_to_rgba(grey, np.full((16, 16, 2), 128, np.uint8), matrix, rng, siting)
        assert (back[..., :3] == grey[..., None]).all() and (back[..., 3] == 255).all()
    else:
        assert y.min() == 16 and y.max() == 235
        lum = np.repeat(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16), 2, axis=0), 2, axis=1)
        back = ym.nv12_to_rgba(lum, np.full((16, 16, 2), 128, np.uint8), matrix, rng, siting)
        assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all()
        assert (back[lum <= 16][:, :3] == 0).all() and (back[lum >= 235][:, :3] == 255).all()


@pytest.mark.parametrize("matrix", ym.MATRICES)
def test_limited_white_and_black(matrix):
    for siting in ym.SITINGS:
        y, uv = ym.rgba_to_nv12(solid(255, 255, 255), matrix, ym.LIMITED, siting)
        assert (y == 235).all() and (uv == 128).all()
        y, uv = ym.rgba_to_nv12(solid(0, 0, 0), matrix, ym.LIMITED, siting)
        assert (y == 16).all() and (uv == 128).all()
        assert (ym.nv12_to_rgba(*grey_nv12(235), matrix, ym.LIMITED, siting)[..., :3] == 255).all()
        assert (ym.nv12_to_rgba(*grey_nv12(16), matrix, ym.LIMITED, siting)[..., :3] == 0).all()


# (Y, Cb, Cr) of 100 % red, green and blue: ITU-R BT.601 and BT.709 8-bit limited-range tables; the full-range ones from
# Y = 255 Kc, C = 128 +- 127.5 scaled by the other two weights, rounded
PRIMARIES = {
    (ym.BT601, ym.LIMITED): [(81, 90, 240), (145, 54, 34), (41, 240, 110)],
    (ym.BT709, ym.LIMITED): [(63, 102, 240), (173, 42, 26), (32, 240, 118)],
    (ym.BT601, ym.FULL): [(76, 85, 255), (150, 44, 21), (29, 255, 107)],
    (ym.BT709, ym.FULL): [(54, 99, 255), (182, 30, 12), (18, 255, 116)],
}


@pytest.mark.parametrize("siting", ym.SITINGS)
@mr
def test_primaries(matrix, rng, siting):
    for colour, want in zip([(255, 0, 0), (0, 255, 0), (0, 0, 255)], PRIMARIES[(matrix, rng)]):
        y, uv = ym.rgba_to_nv12(solid(*colour, 4, 2), matrix, rng, siting)
        assert (y == want[0]).all() and (uv[..., 0] == want[1]).all() and (uv[..., 1] == want[2]).all(), (colour, y[0, 0], uv[0, 0])
        real = [float(v) for v in ym.real_yuv(*colour, matrix, rng)]
        assert all(abs(w - r) <= 0.5 + 1e-9 or (r == 255.0 and w == 255) for w, r in zip(want, real)), (want, real)
        back = ym.nv12_to_rgba(y, uv, matrix, rng, siting)                               # and back to within an LSB or two
        assert np.abs(back[0, 0, :3].astype(int) - np.array(colour)).max() <= 2, (colour, back[0, 0])


# ---- 4. within +-1 LSB of the float64 evaluation for EVERY input: the 14-bit coefficients are off by less than 0.03 LSB in
# all (half a unit of 2^-14 times at most 255 + 2 * 128, three halves for the adjusted ones), the rounding by half an LSB

@mr
def test_every_yuv_triple_within_one_lsb(matrix, rng):
    worst = 0.0
    for cb in range(0, 256, 16):                                                        # 16 slabs of 16 x 256 x 256
        cbs, crs, ys = np.meshgrid(np.arange(cb, cb + 16), np.arange(256), np.arange(256), indexing="ij")
        uv = np.stack([cbs, crs], axis=-1).astype(np.uint8).reshape(16 * 256, 256, 2)
        y = ys.astype(np.uint8).reshape(16 * 256, 256)
        # one quad per triple: the model under REPLICATE on a 2x-repeated plane is the per-sample formula
        got = ym.nv12_to_rgba(np.repeat(np.repeat(y, 2, 0), 2, 1), uv, matrix, rng, ym.REPLICATE)[0::2, 0::2]
        real = ym.real_rgb(y, uv[..., 0], uv[..., 1], matrix, rng)
        for c in range(3):
            worst = max(worst, float(np.abs(got[..., c] - real[c]).max()))
        assert (got[..., 3] == 255).all()
    print(f"NV12 -> RGBA {NAMES[(matrix, rng)]}: largest |model - float64| = {worst:.4f} LSB")
    assert worst <= 1.0
    assert worst <= 0.5 + 0.03                                                          # what the reasoning above gives


@mr
def test_every_rgb_triple_within_one_lsb(matrix, rng):
    worst = [0.0, 0.0, 0.0]
    for b in range(0, 256, 16):
        bs, gs, rs = np.meshgrid(np.arange(b, b + 16), np.arange(256), np.arange(256), indexing="ij")
        flat = np.stack([rs, gs, bs, bs], axis=-1).astype(np.uint8).reshape(16 * 256, 256, 4)
        quads = np.repeat(np.repeat(flat, 2, 0), 2, 1)                                  # one uniform quad per colour
        y, uv = ym.rgba_to_nv12(quads, matrix, rng, ym.REPLICATE)
        assert (y[0::2, 0::2] == y[1::2, 1::2]).all()
        real = ym.real_yuv(flat[..., 0], flat[..., 1], flat[..., 2], matrix, rng)
        for c, got in enumerate((y[0::2, 0::2], uv[..., 0], uv[..., 1])):
            worst[c] = max(worst[c], float(np.abs(got - real[c]).max()))
    print(f"RGBA -> NV12 {NAMES[(matrix, rng)]}: largest |model - float64| = {worst} LSB")
    assert max(worst) <= 1.0
    assert max(worst) <= 0.5 + 0.03


def test_uniform_quads_give_left_what_replicate_gives():
    """On an image of uniform 6 x 2 blocks LEFT's three columns carry one colour, so both sitings agree there -- which extends
    the exhaustive chroma check above to LEFT's weights, shift and rounding constant."""
    rgba = np.repeat(np.repeat(ym.random_rgba(8, 6, 5), 2, axis=0), 6, axis=1)
    for matrix, rng in MATRIX_RANGE:
        a, b = ym.rgba_to_nv12(rgba, matrix, rng, ym.REPLICATE), ym.rgba_to_nv12(rgba, matrix, rng, ym.LEFT)
        assert (a[0] == b[0]).all()
        assert (a[1][:, 1::3] == b[1][:, 1::3]).all() and (a[1][:, 2::3] == b[1][:, 2::3]).all()


# ---- 5. the sitings

@mr
def test_left_on_constant_chroma_equals_replicate(matrix, rng):
    y, _ = ym.random_nv12(18, 6, 3)
    for pair in [(0, 255), (255, 0), (128, 128), (37, 201)]:
        uv = np.broadcast_to(np.array(pair, np.uint8), (3, 9, 2)).copy()
        assert (ym.chroma8(uv[..., 0], ym.LEFT) == ym.chroma8(uv[..., 0], ym.REPLICATE)).all()
        assert (ym.nv12_to_rgba(y, uv, matrix, rng, ym.LEFT) == ym.nv12_to_rgba(y, uv, matrix, rng, ym.REPLICATE)).all()


def test_left_weights_by_hand():
    """A 4 x 4 plane of distinct powers of a base: every weight of every output shows in the sum."""
    c = np.array([[1, 10], [100, 1000]], np.int32)
    got = ym.chroma8(c, ym.LEFT)
    want = np.array([
        # x = 0 (even: 2 C[.][0]), 1 (odd: C[.][0] + C[.][1]), 2 (even: 2 C[.][1]), 3 (odd: C[.][1] twice, clamped)
        [3 * 2 + 2, 3 * 11 + 11, 3 * 20 + 20, 3 * 20 + 20],                             # y = 0: row 0 and row -1 -> 0
        [3 * 2 + 200, 3 * 11 + 1100, 3 * 20 + 2000, 3 * 20 + 2000],                     # y = 1: row 0 and row 1
        [3 * 200 + 2, 3 * 1100 + 11, 3 * 2000 + 20, 3 * 2000 + 20],                     # y = 2: row 1 and row 0
        [3 * 200 + 200, 3 * 1100 + 1100, 3 * 2000 + 2000, 3 * 2000 + 2000],             # y = 3: row 1 and row 2 -> 1
    ], np.int32)
    assert (got == want).all()
    assert (ym.chroma8(c, ym.REPLICATE) == 8 * np.repeat(np.repeat(c, 2, 0), 2, 1)).all()


def test_clamped_edges_at_2x2():
    """One chroma sample, one quad: every neighbour index clamps onto it."""
    for matrix, rng in MATRIX_RANGE:
        y, uv = ym.random_nv12(2, 2, 9)
        uv[0, 0] = (60, 190)
        assert (ym.chroma8(uv[..., 0], ym.LEFT) == 8 * 60).all() and (ym.chroma8(uv[..., 1], ym.LEFT) == 8 * 190).all()
        assert (ym.nv12_to_rgba(y, uv, matrix, rng, ym.LEFT) == ym.nv12_to_rgba(y, uv, matrix, rng, ym.REPLICATE)).all()
        rgba = ym.random_rgba(2, 2, 11)
        _, k = ym.coefficients(matrix, rng)
        p = rgba[..., :3].astype(np.int64)
        s = 3 * (p[0, 0] + p[1, 0]) + (p[0, 1] + p[1, 1])                # column -1 is column 0: weights 3, 1
        cb = int(np.clip(128 + ((k[3] * s[0] + k[4] * s[1] + k[5] * s[2] + (1 << 16)) >> 17), 0, 255))
        cr = int(np.clip(128 + ((k[6] * s[0] + k[7] * s[1] + k[8] * s[2] + (1 << 16)) >> 17), 0, 255))
        got = ym.rgba_to_nv12(rgba, matrix, rng, ym.LEFT)[1]
        assert tuple(got[0, 0]) == (cb, cr)


def test_both_clamps_fire_on_the_shared_random_planes():
    """The random planes the GPU tests use reach below 0 and above 255 before the clamp, in every channel that can."""
    y, uv = ym.random_nv12(18, 6, 1)
    (c_y, c_rv, _, _, c_bu), _ = ym.coefficients(ym.BT601, ym.FULL)
    yy = 8 * c_y * y.astype(np.int64) + (1 << 16)
    cr = ym.chroma8(uv[..., 1], ym.REPLICATE).astype(np.int64) - 1024
    r = (yy + c_rv * cr) >> 17
    assert r.min() < 0 and r.max() > 255
    rgba = ym.random_rgba(18, 6, 1)
    assert (rgba[0, 0, :3] == 0).all() and (rgba[-1, -1, :3] == 255).all()
