"""lfg_upscale_edge's definition on the CPU (tests/edge_model.py): the positions against Python integers, the library's two host
builders against the model's, the weight sum over every shape and every phase, the 32-bit bound on every intermediate, what the
header promises (constants, brackets, steps), and the quality against the separable filters of tests/resample_model.py on rendered
scenes.  CPU only; the library is loaded for its two pure host functions."""
import os

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import edge_model as em
from tests import resample_model as rm

GROWING = [(i, o) for i, o in rm.RATIOS if o >= i] + [(1, 1), (1, 7), (7, 8), (64, 65), (2, 6), (1080, 2160)]
SHAPES = [(1, 1, 4, 3), (5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (24, 16, 24, 16), (33, 5, 65, 9)]


@pytest.fixture(scope="module")
def library():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return capi


@pytest.mark.parametrize("pair", GROWING, ids=["{}-{}".format(*p) for p in GROWING])
def test_positions_are_the_floor_and_its_remainder(pair, library):
    n_in, n_out = pair
    base, frac = em.positions(n_in, n_out)
    for p in range(n_out):
        N, D = (2 * p + 1) * n_in - n_out, 2 * n_out                     # Python integers: // is the floor
        a = N // D
        assert (int(base[p]), int(frac[p])) == (a, 256 * (N - a * D) // D), p
    assert base.min() >= -1 and base.max() <= n_in - 1 and frac.min() >= 0 and frac.max() <= 255
    assert (np.diff(base) >= 0).all() and (np.diff(base) <= 1).all()      # what the kernel's tile rests on
    lib_base, lib_frac = library.upscale_edge_positions(n_in, n_out)
    assert lib_base.dtype == np.int32 and lib_frac.dtype == np.uint8
    assert (lib_base == base).all() and (lib_frac == frac).all()


def test_positions_refuse_what_has_none(library):
    for n_in, n_out in ((0, 4), (4, 0), (2 ** 31, 4)):
        with pytest.raises(capi.LfgError) as e:
            library.upscale_edge_positions(n_in, n_out)
        assert e.value.code == capi.ERR_INVALID


def test_shapes_are_the_models(library):
    table = em.shapes()
    assert table.shape == (16, 33, 5)
    assert table[..., 0].max() <= 2047 and table[..., 2].max() <= 2047 and table[..., 4].max() <= 19508 and np.abs(table).max() < 2 ** 15
    assert table[0, 0].tolist() == [1024, 0, 1024, 2048, 8192]            # flat: the round window, zero at two texels
    got = library.upscale_edge_shapes()
    assert got.dtype == np.int16 and (got == table).all()


def test_the_weight_sum_is_positive_for_every_shape_and_phase():
    """All 16 x 33 shapes x 256 x 256 (fx, fy), step 1: W stays in 3,364 .. 8,356 and the negative weights of a pixel sum to at
    most 3,490 in magnitude (DESIGN.md section 4.25 quotes the three)."""
    table, f = em.shapes(), np.arange(256, dtype=np.int64)
    lo, hi, negative, peaks = 1 << 30, 0, 0, {}
    for k in range(em.DIRECTIONS):
        for q in range(em.STRENGTHS):
            wt = em.weights(table[k, q], f[None, :], f[:, None], peaks)
            W = wt.sum(0)
            lo, hi, negative = min(lo, int(W.min())), max(hi, int(W.max())), max(negative, int(-np.minimum(wt, 0).sum(0).min()))
    print(f"W in {lo} .. {hi}; negative weights sum to at most {negative}; peaks {peaks}")
    assert lo > 0
    assert (lo, hi, negative) == (3364, 8356, 3490)
    assert max(peaks.values()) < 2 ** 31
    assert 2 * 255 * (hi + 2 * negative) + hi < 2 ** 26 and 2 * hi < 2 ** 15       # what the kernel's division rests on


def test_every_intermediate_fits_32_bits_on_binary_noise():
    peaks = {}
    for w, h, ow, oh in SHAPES:
        em.upscale(em.binary_noise(w, h, 100 * w + h), ow, oh, peaks=peaks)
    print(peaks)
    assert len(peaks) >= 18 and max(peaks.values()) < 2 ** 31
    assert peaks["DX"] <= 65536 * 1020 and peaks["2 S + W"] < 2 ** 26


def test_a_constant_frame_stays_constant():
    for w, h, ow, oh in SHAPES:
        for value in (0, 1, 129, 255):
            assert (em.upscale(np.full((h, w, 4), value, np.uint8), ow, oh) == value).all(), (w, h, ow, oh, value)


def test_every_output_lies_within_its_bracket():
    for w, h, ow, oh in SHAPES + [(40, 9, 130, 20)]:
        for frame in (em.binary_noise(w, h, 7 * w + h), em.random_bytes(w, h, 8 * w + h), em.diagonal_edge(w, h)):
            got, (lo, hi) = em.upscale(frame, ow, oh), em.bracket(frame, ow, oh)
            assert (got >= lo).all() and (got <= hi).all(), (w, h, ow, oh)


def test_steps_do_not_overshoot():
    for vertical in (True, False):
        frame = np.full((12, 12, 4), 40, np.uint8)
        if vertical:
            frame[:, 6:] = 200
        else:
            frame[6:] = 200
        for ow, oh in ((24, 24), (18, 18), (25, 13)):
            got = em.upscale(frame, ow, oh)
            assert got.min() == 40 and got.max() == 200, (vertical, ow, oh, got.min(), got.max())
            line = got[oh // 2, :, 0] if vertical else got[:, ow // 2, 0]
            assert (np.diff(line.astype(int)) >= 0).all(), line            # and no ripple: the step rises once


def test_equal_sizes_are_not_the_identity():
    frame = em.binary_noise(24, 16, 3)
    assert (em.upscale(frame, 24, 16) != frame).any()


def test_a_region_is_the_whole_calls():
    frame = em.random_bytes(33, 21, 5)
    whole = em.upscale(frame, 70, 50)
    for x0, y0, w, h in ((0, 0, 9, 7), (61, 43, 9, 7), (30, 11, 17, 3)):
        assert (em.upscale(frame, 70, 50, roi=(x0, y0, w, h)) == whole[y0:y0 + h, x0:x0 + w]).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quality_on_rendered_edges_beats_every_separable_filter(seed):
    """256 x 256 scenes of bars and discs at random angles, rendered at 4 x 4 samples per pixel, box-downscaled 2 : 1 and
    upscaled 2 x again: the PSNR over R, G, B against the rendered truth is strictly above that of each separable filter.  The
    margins this printed are in DESIGN.md section 4.25."""
    truth = em.scene(256, seed)
    small = em.box_down(truth, 2)
    edge = em.psnr(em.upscale(small, 256, 256), truth)
    others = {rm.NAMES[f]: em.psnr(rm.resample(small, 256, 256, f), truth) for f in (rm.BILINEAR, rm.CATMULL_ROM, rm.LANCZOS2, rm.LANCZOS3)}
    print(f"seed {seed}: edge-adaptive {edge:.2f} dB; " + ", ".join(f"{n} {v:.2f}" for n, v in others.items()))
    for name, value in others.items():
        assert edge > value, (name, edge, value)
