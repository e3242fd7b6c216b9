"""The consequences that include/linuxfg_hip.h states for lfg_denoise_temporal, asserted on the CPU model
(tests/denoise_model.py), and the noise figure the stage is built for.  CPU only."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import denoise_cases as dc
from tests import denoise_model as dm

W, H = 64, 48


def zero(w=W, h=H):
    return dc.constant_field(w, h, 0, 0)


@pytest.mark.parametrize("count", dc.COUNTS)
@pytest.mark.parametrize("radius", dc.RADII)
def test_strength_0_and_limit_0_copy(radius, count):
    curr = dc.random_frame(W, H, 1)
    refs = [dc.random_frame(W, H, 2), dc.noisy(curr, 2, 3)][:count]
    mvs = [dc.small_field(W, H, 4), zero()][:count]
    assert (dm.denoise(curr, refs, mvs, radius, 1020, 0, 255) == curr).all()
    assert (dm.denoise(curr, refs, mvs, radius, 1020, 256, 0) == curr).all()


@pytest.mark.parametrize("count", dc.COUNTS)
@pytest.mark.parametrize("radius", dc.RADII)
def test_identical_references_give_curr(radius, count):
    curr = dc.scene(W, H, 5)
    assert (dm.denoise(curr, [curr] * count, [zero()] * count, radius, 32, 256, 255) == curr).all()


@pytest.mark.parametrize("radius", dc.RADII)
def test_an_uncorrelated_reference_is_refused(radius):
    """Random bytes against random bytes (synth's uncorrelated pair, a hash of the position) differ by ~85 levels per channel:
    far above 32 per texel over four channels, even at radius 0, where one texel decides (the smallest cost in this pair is
    asserted, not assumed: 43 at radius 0, 208 and 255 per texel at radius 1 and 2)."""
    curr, ref = synth.make_uncorrelated_pair(W, H)
    cost, n, _ = dm.window_cost(curr, ref, zero(), radius)
    assert (cost >= 32 * n).all()
    assert (dm.denoise(curr, [ref], [zero()], radius, 32, 256, 255) == curr).all()


@pytest.mark.parametrize("radius", dc.RADII)
def test_a_block_that_differs_is_left_alone(radius):
    """The reference is curr except inside a 10 x 10 block of other content: no pixel whose window lies inside the block moves."""
    curr = dc.scene(W, H, 8)
    ref = curr.copy()
    x0, y0 = 20, 15
    ref[y0:y0 + 10, x0:x0 + 10] = curr[y0:y0 + 10, x0:x0 + 10] ^ 0x80            # every channel differs by 128: 512 per texel
    out = dm.denoise(curr, [ref], [zero()], radius, 32, 256, 255)
    inner = (slice(y0 + radius, y0 + 10 - radius), slice(x0 + radius, x0 + 10 - radius))
    assert (out[inner] == curr[inner]).all()
    far = np.ones((H, W), bool)
    far[y0 - radius:y0 + 10 + radius, x0 - radius:x0 + 10 + radius] = False
    assert (out[far] == curr[far]).all()                                       # identical there: out = curr as well


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (37, 23)])
@pytest.mark.parametrize("radius", dc.RADII)
def test_range_and_limit_on_random_frames_and_vectors(radius, w, h):
    rng = np.random.default_rng(100 * w + radius)
    for trial in range(6):
        curr = dc.noisy(dc.scene(w, h, trial), 8, trial + 50) if trial % 2 else dc.random_frame(w, h, trial)
        refs = [dc.noisy(curr, 6, trial + 60), dc.random_frame(w, h, trial + 70)]
        mvs = [dc.small_field(w, h, trial + 80) if trial % 3 else dc.random_field(w, h, trial + 80), dc.outward_field(w, h)]
        mvs[0][0, 0] = (-128, -128)
        tolerance, strength, limit = int(rng.integers(1, 1021)), int(rng.integers(0, 257)), int(rng.integers(0, 256))
        for count in dc.COUNTS:
            out = dm.denoise(curr, refs[:count], mvs[:count], radius, tolerance, strength, limit).astype(np.int64)
            c = curr.astype(np.int64)
            assert (np.abs(out - c) <= limit).all()
            lo, hi = c.copy(), c.copy()
            ys, xs = np.mgrid[0:h, 0:w]
            for ref, mv in zip(refs[:count], mvs[:count]):
                v = mv.astype(np.int64)
                ty, tx = ys + v[..., 1], xs + v[..., 0]
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                there = ref.astype(np.int64)[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]
                lo = np.where(inside[..., None], np.minimum(lo, there), lo)
                hi = np.where(inside[..., None], np.maximum(hi, there), hi)
            assert ((out >= lo) & (out <= hi)).all()


def test_half_and_three_quarters_for_a_perfect_reference():
    """Cost 0: w = strength L / 64, so a_1 = 256 s / (64 + s): 128 at strength 64, 192 at 192."""
    L = np.array([32, 288, 800])
    assert (dm.shares(L, dm.weight(64, L, 0))[1] == 128).all()
    assert (dm.shares(L, dm.weight(192, L, 0))[1] == 192).all()


def recursive_ratio(amplitude, tolerance, strength, frames=9, radius=1, two=False):
    """MSE of the last output against the clean frame over the MSE of its input, the filter fed `frames` noisy frames of one
    clean pattern recursively (refs[0] the previous output); with `two`, the next noisy frame is a second reference."""
    clean = dc.scene(W, H, 11)
    noisy = [dc.noisy(clean, amplitude, 1000 + k) for k in range(frames + 1)]
    out = noisy[0]
    for k in range(1, frames):
        refs = [out, noisy[k + 1]] if two else [out]
        out = dm.denoise(noisy[k], refs, [zero()] * len(refs), radius, tolerance, strength, 255)
    return dc.mse(out, clean) / dc.mse(noisy[frames - 1], clean)


def test_the_noise_figure():
    """+-4 levels on R, G and B of a 64 x 48 pattern, zero vectors, radius 1, tolerance 32, strength 192, nine frames
    recursively: the error against the clean frame falls below 0.30 of the input's.  This model gives 0.218 (an earlier numpy
    sketch of the definition: 0.22)."""
    ratio = recursive_ratio(4, 32, 192)
    print(f"recursive, +-4, strength 192: {ratio:.3f}")
    assert ratio < 0.30


def test_the_other_figures_are_printed():
    """Not bounds, figures (pytest -s shows them): this model gives 0.525 for one pass at strength 64, 0.358 with the next frame
    as a second reference, and 0.903 at +-8 with tolerance 16, where the guard refuses most windows."""
    one = dc.mse(dm.denoise(dc.noisy(dc.scene(W, H, 11), 4, 1001), [dc.noisy(dc.scene(W, H, 11), 4, 1000)], [zero()], 1, 32, 64, 255),
                 dc.scene(W, H, 11)) / dc.mse(dc.noisy(dc.scene(W, H, 11), 4, 1001), dc.scene(W, H, 11))
    two, refused = recursive_ratio(4, 32, 64, frames=2, two=True), recursive_ratio(8, 16, 192)
    print(f"one pass, strength 64: {one:.3f}; two references: {two:.3f}; +-8 at tolerance 16: {refused:.3f}")
    assert two < one < 1.0            # (a mean of three independent samples has less noise than one of two, and that than one)
