"""The float64 model of shaders/scale.comp (oracle/scale_f64.py): its own known answers, the C oracle held to it, and
the error budget that turns the GPU tests' bar (kernel within eps of the model, tests/test_gpu_parity.py) into +-1 LSB
against the shader for every input.  CPU only.

The budget: with K the kernel's value before rounding, O the shader's and V the model's,
  |K - V| <= eps (GPU tests, eps = 1e-3),  |O - V| <= B + eps_o (B = subtexel_bound, eps_o the oracle's fp32 error),
and |K - O| < 1 makes the two rounded bytes differ by at most 1 (clamping to 0..255 keeps that).  So eps + B + eps_o < 1
proves the north-star bar at a size, whatever the content.  B per size pair (LSB):
  540p -> 1080p 0.046   1080p -> 4K 0.084   4K -> 8K 0.175    720p -> 1080p 0.049
  1440p -> 4K   0.104   720p -> 4K  0.050   4K -> 1080p 0.207 8K -> 16K 0.333
and below 1 - 2e-3 for every shape of the GPU tests' sweeps (test_error_budget_below_one_lsb).
"""
import numpy as np
import pytest

from oracle import scale_f64 as m

EPS_ORACLE = 1e-4          # the C oracle's own fp32 rounding, in LSB


def check_oracle_against_model(O, V, B):
    """The C oracle's bytes O against the model: within half an LSB plus B everywhere, and equal to rint(V) wherever V
    is further than B from a rounding boundary.  Returns the fraction of bytes != rint(V)."""
    c = np.clip(V, 0.0, 255.0)
    d = np.abs(O.astype(np.float64) - c)
    assert d.max() <= 0.5 + B + EPS_ORACLE, f"|O - V| = {d.max():.4f} > 0.5 + {B:.4f} at {np.unravel_index(d.argmax(), d.shape)}"
    r = np.rint(c)
    far = ~m.near_half(V, B + EPS_ORACLE)
    bad = far & (O != r)
    assert not bad.any(), f"{int(bad.sum())} bytes away from a tie differ from rint(V), first at {np.argwhere(bad)[0]}"
    return float((O != r).mean())


# ------------------------------------------------------------------ the model's own known answers

def test_constant_frame_gives_the_constant():
    f = np.empty((9, 13, 4), np.uint8)
    f[...] = (10, 200, 77, 255)
    for ow, oh in [(26, 18), (13, 9), (31, 20), (7, 5), (1, 1)]:
        V = m.scale_f64(f, ow, oh)
        assert np.abs(V - f[0, 0]).max() < 1e-9, (ow, oh)


def test_same_size_gives_the_input_back():
    f = np.random.default_rng(5).integers(0, 256, (23, 37, 4), dtype=np.uint8)
    V = m.scale_f64(f, 37, 23)
    assert np.abs(V - f).max() < 1e-3
    assert (np.rint(V) == f).all()


def test_2x_phase_rows_are_s_kat3():
    """S-KAT3 (tests/test_oracle_kat.py): the two phases of an exact 2x, raw weights summing to 0.996971."""
    raw = np.array([0.030021, -0.132871, 0.890067, 0.270190, -0.067791, 0.007356])
    for n in (960, 1920, 3840):
        s, w, kept, _ = m.axis_taps(n, 2 * n)
        assert s[200] == 100 - 3 and s[201] == 100 - 2 and kept[200:202].all()
        assert np.allclose(w[201], raw / raw.sum(), atol=2e-6)           # f = 0.25
        assert np.allclose(w[200], raw[::-1] / raw.sum(), atol=2e-6)     # f = 0.75


def test_impulse_gives_the_outer_product_of_the_rows():
    n = 16
    f = np.zeros((n, n, 4), np.uint8)
    f[8, 9] = 255
    V = m.scale_f64(f, 2 * n, 2 * n)
    sx, wx, _, _ = m.axis_taps(n, 2 * n)
    want = np.zeros((2 * n, 2 * n))
    for oy in range(2 * n):
        for ox in range(2 * n):
            ky, kx = 8 - sx[oy], 9 - sx[ox]
            if 0 <= ky < 6 and 0 <= kx < 6:
                want[oy, ox] = 255.0 * wx[oy, ky] * wx[ox, kx]
    assert np.abs(V - want[..., None]).max() < 1e-9
    assert V.min() < -10 and V.max() > 200                 # negative lobes stay in the model (clipped only when rounded)


@pytest.mark.parametrize("n_in,n_out", [(1, 7), (2, 4), (5, 64), (37, 53), (80, 40), (33, 1), (1921, 3842), (3840, 1920)])
def test_weight_rows_sum_to_one_and_skipped_taps_are_zero(n_in, n_out):
    s, w, kept, a = m.axis_taps(n_in, n_out)
    assert np.abs(w.sum(1) - 1.0).max() < 1e-12
    assert (w[~kept] == 0).all() and (a[~kept] == 0).all()
    idx = s[:, None] + np.arange(6)[None, :]
    assert ((idx[kept] >= 0) & (idx[kept] < n_in)).all()      # a kept tap is always a texel of the image


# ------------------------------------------------------------------ the C oracle against the model

SMALL = [((64, 36), (128, 72)), ((200, 75), (400, 150)), ((67, 29), (134, 58)), ((37, 23), (53, 41)),
         ((80, 48), (40, 24)), ((33, 17), (33, 17)), ((5, 3), (64, 40))]        # test_scale_matches_oracle's shapes


@pytest.mark.parametrize("in_wh,out_wh", SMALL)
def test_oracle_within_the_bound_of_the_model_small(oracle, in_wh, out_wh):
    B = m.subtexel_bound(in_wh, out_wh)
    for name, f in m.contents(*in_wh, seed=in_wh[0] * 7 + in_wh[1], seam_rows=range(2, in_wh[1], 7)).items():
        check_oracle_against_model(oracle.scale(f, *out_wh), m.scale_f64(f, *out_wh), B)


def test_oracle_within_the_bound_of_the_model_config1(oracle):
    """Config 1 (960x540 -> 1920x1080) in full, every content."""
    B = m.subtexel_bound((960, 540), (1920, 1080))
    fracs = {}
    for name, f in m.contents(960, 540, seed=540, seam_rows=range(2, 540, 67)).items():
        fracs[name] = check_oracle_against_model(oracle.scale(f, 1920, 1080), m.scale_f64(f, 1920, 1080), B)
    print("oracle bytes != rint(V) at 540p -> 1080p:", {k: f"{v:.3%}" for k, v in fracs.items()})
    assert fracs["noise"] < 0.01


def test_oracle_within_the_bound_of_the_model_1080p_to_4k_rois(oracle):
    B = m.subtexel_bound((1920, 1080), (3840, 2160))
    rois = [(0, 0, 96, 40), (3744, 2120, 3840, 2160), (1800, 1000, 1960, 1040), (0, 2100, 64, 2160), (3700, 0, 3840, 24)]
    for name, f in m.contents(1920, 1080, seed=1080, seam_rows=range(2, 1080, 135)).items():
        for roi in rois:
            x0, y0, x1, y1 = roi
            O = oracle.scale(f, 3840, 2160, roi=roi)[y0:y1, x0:x1]
            check_oracle_against_model(O, m.scale_f64(f, 3840, 2160, roi=roi), B)


# ------------------------------------------------------------------ the error budget

BUDGET = {((960, 540), (1920, 1080)): 0.046, ((1920, 1080), (3840, 2160)): 0.084, ((3840, 2160), (7680, 4320)): 0.175,
          ((1280, 720), (1920, 1080)): 0.049, ((2560, 1440), (3840, 2160)): 0.104, ((1280, 720), (3840, 2160)): 0.050,
          ((3840, 2160), (1920, 1080)): 0.207, ((7680, 4320), (15360, 8640)): 0.333}


def test_error_budget_below_one_lsb():
    """B + eps + eps_o < 1 at the listed size pairs (figures as in the module docstring) and at every shape the GPU tests
    hold to the model: there the kernels' +-1 LSB against the shader holds for all content, not only the content tried."""
    for pair, want in BUDGET.items():
        B = m.subtexel_bound(*pair)
        assert abs(B - want) < 1e-3, (pair, B)
        assert B + 2e-3 < 1.0
    shapes = [((w, h), (2 * w, 2 * h)) for w, h in m.sweep_2x_shapes()] + m.GENERIC_SHAPES + SMALL
    shapes += [((3840, 2160), (7680, 4320)), ((64, 40), (128, 80))]
    for in_wh, out_wh in shapes:
        assert m.subtexel_bound(in_wh, out_wh) + 2e-3 < 1.0, (in_wh, out_wh)
