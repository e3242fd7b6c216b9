"""The CPU model of lfg_motion_subpel and lfg_interpolate_compensated_subpel (tests/subpel_model.py) held to the header:
hand-worked answers, the recovery of a fractional pan, the anchor (with mvq = 4 mv the route is the integer one, byte for
byte), what the fraction buys on a fractional pan, and the power of the shared cases against the model's mutants.  And what
lfg_host refuses next to --subpel-vectors, before it looks for a device.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import mc_model as mc
from tests import subpel_cases as sc
from tests import subpel_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linux-fg_amd", "lfg_host")


@pytest.mark.parametrize("name", sorted(sc.KNOWN))
def test_known_answers(name):
    prev, curr, mv, radius, want = sc.KNOWN[name]()
    got = sm.refine(prev, curr, mv, radius)
    bad = [(q, tuple(int(c) for c in got[q[1], q[0]]), w) for q, w in want.items() if tuple(got[q[1], q[0]]) != w]
    assert not bad, bad[:4]


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_every_output_is_within_three_quarters_and_in_range(radius):
    prev, curr, mv = sc.random_vectors(41, 23, 5)
    got = sm.refine(prev, curr, mv, radius).astype(int)
    v4 = 4 * np.maximum(mv.astype(int), -127)
    assert np.abs(got - v4).max() <= 3
    assert np.abs(got).max() <= sm.LIMIT


@pytest.mark.parametrize("wq", sc.PANS)
def test_recovery_of_a_fractional_pan(wq):
    """fractional_pan(96, 64, wq) with the rounded integer vector everywhere: the share of pixels at least 10 px from the
    border at which the model returns wq.  Observed on the model:
        wq          radius 1       radius 2
        (10, -6)    100 %          100 %
        (6, 2)      100 %          100 %
        (-5, 3)     3343 / 3344    100 %
        (7, 9)      100 %          100 %
    The one pixel is (82, 48) of the (-5, 3) pan at radius 1, where the model returns (-5, 5).  The truth costs 0 there, but
    the search is two greedy stages, not all 49 candidates: over that pixel's nine texels a half-pixel step with dy = +2 costs
    less than every half-pixel step next to the truth (600 at best), and stage 2 reaches only +-1 around stage 1's winner.
    Over 25 texels stage 1 ends next to the truth.  The definition is followed; the assertion is
    the measured share."""
    prev, curr, _ = sc.fractional_pan(96, 64, wq)
    mv = sc.pan_vectors(96, 64, wq)
    for radius in (1, 2):
        hit = (sc.interior(sm.refine(prev, curr, mv, radius)) == np.array(wq)).all(-1)
        missed = int((~hit).sum())
        print(wq, radius, f"{hit.sum()} / {hit.size}")
        assert missed == (1 if (wq, radius) == ((-5, 3), 1) else 0), (wq, radius, missed, np.argwhere(~hit)[:4].tolist())


@pytest.mark.parametrize("match_sad", sc.MATCH_SADS)
def test_t1_gives_curr(match_sad):
    for i, (w, h) in enumerate([(1, 1), (7, 5), (50, 40)]):
        prev, curr, mvq = sc.random_mvq(w, h, 20 + i)
        assert (sm.interpolate(prev, curr, mvq, 1.0, match_sad) == curr).all()


def test_zero_fraction_anchor():
    """With mvq = 4 mv the sub-pixel route is lfg_interpolate_compensated, byte for byte: on small scenes with random and
    mostly-pan vectors, the hand-made mc_* cases and a dense random field, at match_sad 1020 and at factors 0 .. 1."""
    for name, prev, curr, mv in sc.anchor_inputs():
        mvq = 4 * mv.astype(np.int16)
        for t in sc.FACTORS:
            want = mc.interpolate_compensated(prev, curr, mv, t, 1020)
            got = sm.interpolate(prev, curr, mvq, t, 1020)
            assert (got == want).all(), (name, t, int((got != want).any(-1).sum()))


@pytest.mark.parametrize("match_sad", [0, 48])
def test_zero_fraction_anchor_at_tighter_gates(match_sad):
    for name, prev, curr, mv in sc.anchor_inputs():
        mvq = 4 * mv.astype(np.int16)
        for t in (0.25, 0.7):
            assert (sm.interpolate(prev, curr, mvq, t, match_sad) == mc.interpolate_compensated(prev, curr, mv, t, match_sad)).all(), (name, t)


def test_collision_is_decided_by_the_quarter_pixel_order():
    prev, curr, mvq, (x, y), winner = sc.collision()
    K = sm.keys(prev, curr, mvq, sc.COLLISION_FACTOR, 0)
    assert int(K[y, x]) == sm.key(*winner)
    assert int(K[4, 6]) == sm.HOLE and int(K[4, 7]) == sm.HOLE                  # both sources moved away
    mvq[4, 6], mvq[4, 7] = mvq[4, 7].copy(), mvq[4, 6].copy()                 # the vectors swapped: (6, 4) lands on (4, 4), (7, 4) on (6, 4)
    K = sm.keys(prev, curr, mvq, sc.COLLISION_FACTOR, 0)
    assert int(K[4, 4]) == sm.key(-11, 0) and int(K[4, 6]) == sm.key(-9, 0) and int(K[y, x]) == sm.key(0, 0)


def test_revealed_content_comes_from_curr_and_covered_from_prev():
    prev, curr, mvq, obj = sc.revealed_and_covered()
    out = sm.interpolate(prev, curr, mvq, 0.5, 0)
    assert (out[2, 5] == obj).all()
    assert (out[2, 4] == curr[2, 4]).all() and (out[2, 6] == prev[2, 6]).all()


def sse(a, b):
    d = sc.interior(a).astype(np.int64) - sc.interior(b).astype(np.int64)
    return int((d * d).sum())


def test_quality_on_a_fractional_pan():
    """fractional_pan(96, 64, (10, -6)) at t = 0.5, default gate: the chain through both models (subpel at radius 1, then the
    sub-pixel compensated model) against the integer chain (mc_model on the rounded vectors), both against the true middle
    frame on the interior.  Measured on the models: squared error 13,676,023 -> 1,067,503 (18.0 ->
    29.1 dB), pixels that pass the gate 25.5 % -> 100 %."""
    wq = (10, -6)
    prev, curr, middle = sc.fractional_pan(96, 64, wq)
    mv = sc.pan_vectors(96, 64, wq)
    mvq = sm.refine(prev, curr, mv, 1)
    integer = mc.interpolate_compensated(prev, curr, mv, 0.5)
    subpel = sm.interpolate(prev, curr, mvq, 0.5)
    pass_integer = sc.interior(sm.gate(prev, curr, 4 * mv.astype(np.int16))).mean()
    pass_subpel = sc.interior(sm.gate(prev, curr, mvq)).mean()
    n = sc.interior(middle).size
    psnr = [10 * np.log10(255.0 ** 2 * n / e) for e in (sse(integer, middle), sse(subpel, middle))]
    print(f"sse {sse(integer, middle)} -> {sse(subpel, middle)}, psnr {psnr[0]:.1f} -> {psnr[1]:.1f} dB, gate {pass_integer:.3f} -> {pass_subpel:.3f}")
    assert sse(subpel, middle) < sse(integer, middle)
    assert pass_subpel > pass_integer


def _model_outputs(mutant):
    """Everything the shared cases ask of the model, under one mutant or none."""
    out = []
    for name in sorted(sc.KNOWN):
        prev, curr, mv, radius, _ = sc.KNOWN[name]()
        out.append(sm.refine(prev, curr, mv, radius, mutant))
    for wq in sc.PANS:
        prev, curr, _ = sc.fractional_pan(96, 64, wq)
        out.append(sm.refine(prev, curr, sc.pan_vectors(96, 64, wq), 1, mutant))
    prev, curr, mvq = sc.random_mvq(65, 5, 11)
    out.append(sm.interpolate(prev, curr, mvq, 0.5, 1020, mutant))
    return out


@pytest.mark.parametrize("mutant", sm.MUTANTS)
def test_shared_cases_tell_the_mutants_from_the_model(mutant):
    """Each rewrite of tests/subpel_model.c changes some answer on the cases the GPU tests run: the tie order on
    fraction_tie_* (v is not 0 there), the rounded integer part and stage 2's centre on the pans, the + 7 on `rounding`."""
    model, other = _model_outputs(None), _model_outputs(mutant)
    differ = [i for i, (a, b) in enumerate(zip(model, other)) if (a != b).any()]
    print(mutant, differ)
    assert differ, mutant
    named = dict(zip(sorted(sc.KNOWN), range(len(sc.KNOWN))))
    if mutant == "SHORTEST_W":
        assert named["fraction_tie_dy"] in differ
    if mutant == "ROUND_7":
        assert named["rounding"] in differ


# ---- lfg_host --subpel-vectors: the combinations it refuses, before a device context is made

@pytest.fixture(scope="module")
def host_binary():
    if not os.path.exists(HOST):
        import __graft_entry__ as entry
        entry.build()
    return HOST


@pytest.mark.parametrize("options,clash", [
    ((), "--interpolator shader"),
    (("--interpolator", "shader"), "--interpolator shader"),
    (("--interpolator", "compensated", "--generation", "extrapolate"), "--generation extrapolate"),
    (("--interpolator", "compensated", "--bidirectional", "2"), "--bidirectional"),
    (("--interpolator", "compensated", "--protect-static", "8"), "--protect-static"),
    (("--interpolator", "compensated", "--hole-reach", "32"), "--hole-reach"),
    (("--interpolator", "compensated", "--ranks", "2", "--rank", "0", "--comm-file", "unused"), "--ranks"),
])
def test_host_refuses_the_combinations(host_binary, options, clash):
    p = subprocess.run([host_binary, "--input-width", "64", "--input-height", "36", "--frames", "2", "--quiet", "--subpel-vectors", "1", *options],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stdout == "", (p.returncode, p.stdout, p.stderr)
    assert "--subpel-vectors cannot be combined with " + clash in p.stderr, p.stderr


@pytest.mark.parametrize("value", ["-2", "3", "x", ""])
def test_host_refuses_a_bad_radius(host_binary, value):
    p = subprocess.run([host_binary, "--input-width", "64", "--input-height", "36", "--interpolator", "compensated", "--subpel-vectors", value],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--subpel-vectors" in p.stderr, (p.returncode, p.stderr)
