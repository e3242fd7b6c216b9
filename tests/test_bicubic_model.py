"""The bicubic fetch on the CPU: lfg_sampling_weights against the rational rule, the model (tests/bicubic_model.py) against the
anchors the header draws from the definition, the bounds the header states, the shared cases' coverage of the phases, the
mutants, and what the fetch buys on DESIGN.md section 4.20's scene.  CPU only."""
import os

import numpy as np
import pytest

from tests import bicubic_cases as bc
from tests import bicubic_model as bm
from tests import cases, mc_model, subpel_cases, subpel_model


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as entry
    from linux_fg_amd import capi as c
    if not os.path.exists(c.LIB_PATH):
        entry.build()
    return c


def rule(phi):
    """Wt[phi] from the header's words, in Python integers (// is the floor)."""
    n = [-4096 * phi + 128 * phi ** 2 - phi ** 3, 524288 - 320 * phi ** 2 + 3 * phi ** 3, 4096 * phi + 256 * phi ** 2 - 3 * phi ** 3,
         -64 * phi ** 2 + phi ** 3]
    assert sum(n) == 524288
    w = [(v + 16) // 32 for v in n]
    k = 1 if phi <= 32 else 2
    w[k] = 16384 - sum(w[i] for i in range(4) if i != k)
    return w


def test_weights_are_the_rule(capi):
    want = np.array([rule(phi) for phi in range(64)])
    got = capi.sampling_weights()
    assert got.dtype == np.int16 and (got == want).all()
    assert (bm.weights() == want).all()
    for phi, row in ((0, (0, 16384, 0, 0)), (16, (-1152, 14208, 3712, -384)), (32, (-1024, 9216, 9216, -1024)), (63, (-2, 136, 16374, -124))):
        assert tuple(got[phi]) == row
    assert (got.astype(np.int64).sum(axis=1) == 16384).all()
    for phi in range(1, 64):
        assert (got[64 - phi] == got[phi][::-1]).all(), phi
    assert np.abs(got.astype(np.int64)).sum(axis=1).max() <= 20480
    assert got.min() == -1213
    assert capi.load().lfg_sampling_weights(None) != 0


def test_phase_is_truncated_and_reaches_64_below_zero():
    assert bm.phases_of(0.5 + 63.99 / 64, 0.5 + 0.999 / 64) == (63, 0)
    # u = -2^-25 is a float; u - floorf(u) = 1 - 2^-25 rounds to 1.0f: phase 64, whose row is the texel to the right
    tiny = float(np.float32(0.5) - np.float32(2.0 ** -25))
    assert bm.phases_of(tiny, 0.5) == (64, 0)
    img = np.random.default_rng(1).integers(0, 256, (3, 4, 4)).astype(np.uint8)
    assert (bm.body(img, -1, 1, 64, 0) == 256 * img[1, 0].astype(np.int32)).all()


# ---- anchor 1: integer positions give the bilinear routes' bytes

@pytest.mark.parametrize("name,prev,curr,mv", subpel_cases.anchor_inputs(), ids=[a[0] for a in subpel_cases.anchor_inputs()])
def test_t0_and_t1_equal_the_bilinear_routes(name, prev, curr, mv):
    for field in (mv, 4 * mv.astype(np.int16)):
        for sad in (0, 48, 1020):
            for t in (0.0, 1.0):
                assert (bm.interpolate(prev, curr, field, t, sad) == bm.bilinear(prev, curr, field, t, sad)).all(), (t, sad, field.dtype)
            assert (bm.interpolate(prev, curr, field, 1.0, sad) == curr).all()


@pytest.mark.parametrize("v", [(2, -4), (-6, 0), (0, 0), (126, -126)])
def test_uniform_even_vector_at_half_equals_the_bilinear_routes(v):
    prev, curr = cases.small_scene(65, 21, 5)
    mv = np.zeros((21, 65, 2), np.int8)
    mv[...] = v
    for sad in (0, 48, 1020):
        want = mc_model.interpolate_compensated(prev, curr, mv, 0.5, sad)
        assert (bm.interpolate(prev, curr, mv, 0.5, sad) == want).all()
        assert (bm.interpolate(prev, curr, 4 * mv.astype(np.int16), 0.5, sad) == want).all()


def test_integer_phases_give_the_texel_bit_for_bit():
    img = np.random.default_rng(2).integers(0, 256, (5, 7, 4)).astype(np.uint8)
    img[2, 3] = (0, 1, 254, 255)
    for y in range(5):
        for x in range(7):
            assert (bm.body(img, x, y, 0, 0) == 256 * img[y, x].astype(np.int32)).all()
            got = bm.fetch(img, x + 0.5, y + 0.5)
            assert (got.view(np.uint32) == (img[y, x].astype(np.float32) / np.float32(255.0)).view(np.uint32)).all()


# ---- anchor 2: a constant frame stays constant at every phase

@pytest.mark.parametrize("value", [0, 1, 127, 200, 255])
def test_constant_frame_stays_constant_at_every_phase(value):
    img = np.full((4, 4, 4), value, np.uint8)
    for phiy in range(65):
        for phix in range(65):
            assert (bm.body(img, 1, 1, phix, phiy) == 256 * value).all(), (phix, phiy)
    const = np.full((9, 33, 4), value, np.uint8)
    mvq = np.random.default_rng(value).integers(-128, 128, (9, 33, 2)).astype(np.int16)
    assert (bm.interpolate(const, const, mvq, bc.PHASE_FACTOR, 1020) == value).all()


# ---- anchor 3: the step

def test_step_overshoots_and_the_clamp_engages():
    img = bm.step(8, 4, 40, 200)                                   # the edge between columns 3 and 4
    got = [int(bm.body(img, i, 1, 32, 0)[0]) for i in (2, 3, 4)]   # half a pixel off: between 2|3, 3|4, 4|5
    assert got == [256 * 30, 256 * 120, 256 * 210]
    hard = bm.step(8, 4, 0, 255)
    assert [int(bm.body(hard, i, 1, 32, 0)[0]) for i in (2, 3, 4)] == [0, 32640, 65280]
    free = [int(bm.body(hard, i, 1, 32, 0, mutant="NO_CLAMP")[0]) for i in (2, 3, 4)]
    assert free[0] < 0 and free[2] > 65280 and free[1] == 32640
    assert bm.fetch(hard, 5.0, 1.5)[0] == 1.0 and bm.fetch(hard, 3.0, 1.5)[0] == 0.0


# ---- the bounds the header states

def test_bounds_of_h_and_s_over_the_checkerboard():
    board = bm.checkerboard(6, 6)
    ext = np.array([0, 0, 0, 0], np.int32)
    for i, j in ((2, 2), (3, 2), (0, 0), (5, 5)):                  # both parities; two corners, where the footprint clamps
        for phiy in range(64):
            for phix in range(64):
                p = bm.body(board, i, j, phix, phiy, extremes=ext)
                assert (p >= 0).all() and (p <= bm.P_MAX).all()
    print("h_r in", ext[:2].tolist(), "s in", ext[2:].tolist())
    assert ext[0] < 0, "the checkerboard must drive h_r below zero"
    assert max(-ext[0], ext[1]) <= 40800
    assert max(-int(ext[2]), int(ext[3])) <= 835584000


# ---- the shared cases

def test_shared_cases_hit_every_phase_on_both_axes():
    count = np.zeros((2, 65), np.uint32)
    for name, prev, curr, field in bc.all_cases(sizes=[(65, 5), (97, 61)]):
        for t in bc.FACTORS + [bc.PHASE_FACTOR]:
            bm.interpolate(prev, curr, field, t, 1020, phases=count)
    missing = [(axis, phi) for axis in range(2) for phi in range(64) if count[axis, phi] == 0]
    assert not missing, missing


def test_the_round_factors_alone_would_not():
    """Why PHASE_FACTOR is among the shared factors: quarter-pixel vectors at 0, 0.25, 0.3, 0.5, 0.7 and 1 reach fewer phases."""
    count = np.zeros((2, 65), np.uint32)
    prev, curr, mvq, _ = bc.scene("dense", 97, 61, 3)
    for t in bc.FACTORS:
        bm.interpolate(prev, curr, mvq, t, 1020, phases=count)
    assert (count[:, :64] == 0).any()


MUTANT_CASES = {"TRUNC_SHIFT": "checkerboard", "ROUND_PHASE": "dense", "NO_CLAMP": "step"}


@pytest.mark.parametrize("mutant", bm.MUTANTS)
def test_named_cases_tell_the_mutants_from_the_model(mutant):
    prev, curr, mvq, mv = bc.scene(MUTANT_CASES[mutant], 97, 61, 11)
    differs = 0
    for field in (mvq, mv):
        for t in (0.3, 0.5, bc.PHASE_FACTOR):
            K = bm.keys(prev, curr, field, t, 1020)
            differs += int((bm.sample(prev, curr, field, K, t, 1020) != bm.sample(prev, curr, field, K, t, 1020, mutant=mutant)).any())
    assert differs, f"{mutant} passes for the model on the {MUTANT_CASES[mutant]} case"


def test_the_remainder_is_zero_so_its_tap_cannot_show():
    """The fourth rewrite, the remainder of 16384 on the other centre tap, is no mutant: the four rounded weights sum to 16384 at
    every phase already.  Modulo 32 the numerators are -r, 3r, -3r, r with r = phi^3; x and -x round to opposite integers unless
    x is half-way, which needs r or 3r = 16 mod 32, and a cube is 0, 8, 24 or odd there.  So the rule's last step changes
    nothing, no case can tell the two taps apart, and the model with BICUBIC_MUTANT_WRONG_TAP has the same table."""
    for phi in range(65):
        n = [-4096 * phi + 128 * phi ** 2 - phi ** 3, 524288 - 320 * phi ** 2 + 3 * phi ** 3, 4096 * phi + 256 * phi ** 2 - 3 * phi ** 3,
             -64 * phi ** 2 + phi ** 3]
        assert sum((v + 16) // 32 for v in n) == 16384, phi
    assert (bm.weights("WRONG_TAP") == bm.weights()).all()


def test_roi_is_the_frames_own_pixels():
    prev, curr, mvq, mv = bc.scene("full_range", 97, 61, 4)
    for field in (mvq, mv):
        whole = bm.interpolate(prev, curr, field, 0.3)
        assert (bm.interpolate(prev, curr, field, 0.3, roi=(40, 20, 33, 17)) == whole[20:37, 40:73]).all()


# ---- what it buys

def test_quality_on_the_fractional_pan():
    """DESIGN.md section 4.20's scene with the true quarter-pixel field, t = 0.5, default gate, interior 10 px, against the true
    middle frame: the bicubic fetch must at least halve the bilinear route's squared error (a prototype of the fetch alone
    measured 6.2 x; the factor 2 leaves room for what the gate, the projection and the holes add)."""
    prev, curr, mvq, middle = bc.quality_case()
    bilinear = bc.squared_error(subpel_model.interpolate(prev, curr, mvq, 0.5), middle)
    bicubic = bc.squared_error(bm.interpolate(prev, curr, mvq, 0.5), middle)
    n = subpel_cases.interior(middle).size
    psnr = lambda e: 10 * np.log10(255.0 ** 2 * n / e)
    print(f"squared error: bilinear {bilinear} ({psnr(bilinear):.2f} dB), bicubic {bicubic} ({psnr(bicubic):.2f} dB), {bilinear / bicubic:.2f} x")
    assert 2 * bicubic <= bilinear
