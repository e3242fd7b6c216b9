"""Known answers for the CPU model of lfg_frame_halve and lfg_motion_expand (tests/expand_model.py): a slow numpy restatement
of the definition, the identities the header states, the pyramid's level rule, the pan results that motivate the route, and
the mutants of the model, each told from it by a named case of tests/expand_cases.py."""
import numpy as np
import pytest

from tests import expand_cases as xc
from tests import expand_model as xm
from tests import mc_model as mc
from tests import pyramid_model as pm
from tests.cases import textured

RADII = [0, 1, 2]


# ---- the definition once more, slowly: cost, key, the two steps

def cost(prev, curr, x, y, v, radius):
    h, w = prev.shape[:2]
    s = 0
    for ry in range(y - radius, y + radius + 1):
        for rx in range(x - radius, x + radius + 1):
            if 0 <= rx < w and 0 <= ry < h:
                px, py = rx + v[0], ry + v[1]
                p = prev[py, px].astype(int) if 0 <= px < w and 0 <= py < h else np.zeros(4, int)
                s += int(np.abs(curr[ry, rx].astype(int) - p).sum())
    return s


def slow_expand(prev, curr, low, radius):
    h, w = prev.shape[:2]
    hl, wl = low.shape[:2]
    clamp = lambda c: max(-127, min(127, c))
    out = np.zeros((h, w, 2), np.int8)
    for y in range(h):
        for x in range(w):
            key = lambda v: (cost(prev, curr, x, y, v, radius), v[0] ** 2 + v[1] ** 2, v[1], v[0])
            ns = [(x // 2 + a, y // 2 + b) for b in (-1, 0, 1) for a in (-1, 0, 1)]
            first = [(clamp(2 * int(low[ny, nx, 0])), clamp(2 * int(low[ny, nx, 1]))) for nx, ny in ns if 0 <= nx < wl and 0 <= ny < hl]
            wv = min(first, key=key)
            out[y, x] = min([(clamp(wv[0] + dx), clamp(wv[1] + dy)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], key=key)
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (17, 9), (33, 17)])
def test_c_model_equals_the_slow_restatement(w, h):
    rng = np.random.default_rng(100 * w + h)
    wl, hl = xm.low_size(w, h)
    prev = textured(w, h, w)
    curr = np.clip(prev.astype(int) + rng.integers(-9, 10, prev.shape), 0, 255).astype(np.uint8)
    small = rng.integers(-3, 4, (hl, wl, 2)).astype(np.int8)
    wild = rng.integers(-128, 128, (hl, wl, 2)).astype(np.int8)
    wild.reshape(-1)[:2] = (-128, 127)
    for radius in RADII if w < 33 else [1]:
        for low in (small, wild):
            got, want = xm.expand(prev, curr, low, radius), slow_expand(prev, curr, low, radius)
            assert (got == want).all(), (radius, np.argwhere((got != want).any(-1))[:3].tolist())


# ---- the identities of the header

@pytest.mark.parametrize("radius", RADII)
def test_uniform_field_gives_the_best_of_its_doubled_vector_and_the_steps_around_it(radius):
    w, h = 23, 15
    prev, curr = textured(w, h, 7), textured(w, h, 8)
    for v in ((2, -3), (-128, 127), (127, -128), (64, -64), (0, 0)):
        low = np.zeros(xm.low_size(w, h)[::-1] + (2,), np.int8)
        low[...] = v
        got = xm.expand(prev, curr, low, radius)
        d = [max(-127, min(127, 2 * c)) for c in v]
        for x, y in ((0, 0), (w - 1, h - 1), (11, 7), (22, 0)):
            steps = [(max(-127, min(127, d[0] + dx)), max(-127, min(127, d[1] + dy))) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            want = min(steps, key=lambda u: (cost(prev, curr, x, y, u, radius), u[0] ** 2 + u[1] ** 2, u[1], u[0]))
            assert tuple(int(c) for c in got[y, x]) == want, (v, x, y)


@pytest.mark.parametrize("radius", RADII)
def test_every_output_component_lies_within_127(radius):
    w, h = 41, 27
    rng = np.random.default_rng(radius)
    low = rng.integers(-128, 128, xm.low_size(w, h)[::-1] + (2,)).astype(np.int8)
    low[0, 0], low[1, 1] = (-128, -128), (127, 127)
    got = xm.expand(textured(w, h, 20), textured(w, h, 21), low, radius)
    assert got.min() >= -127 and got.max() <= 127


def test_roi_equals_whole_frame():
    w, h = 71, 45
    rng = np.random.default_rng(4)
    prev, curr = textured(w, h, 12), textured(w, h, 13)
    low = rng.integers(-20, 21, xm.low_size(w, h)[::-1] + (2,)).astype(np.int8)
    for radius in RADII:
        whole = xm.expand(prev, curr, low, radius)
        for x, y, rw, rh in ((0, 0, 9, 7), (62, 38, 9, 7), (21, 17, 30, 12)):
            assert (xm.expand(prev, curr, low, radius, roi=(x, y, rw, rh)) == whole[y:y + rh, x:x + rw]).all()


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 3), (17, 9), (33, 17), (96, 64), (257, 131)])
def test_halve_is_the_pyramids_level_rule(w, h):
    img = textured(w, h, 1000 * w + h)
    got = xm.halve(img)
    assert got.shape == ((h + 1) // 2, (w + 1) // 2, 4)
    assert (got == pm.reduce(img)).all()
    assert (got == pm.pyramid(img, 1)[1]).all()


def test_halve_rounds_half_up_and_clamps_at_odd_edges():
    img = np.zeros((3, 3, 4), np.uint8)
    img[0, 0], img[0, 1], img[2, 2] = 1, 1, 255            # (1 + 1 + 0 + 0 + 2) >> 2 = 1; the corner texel four times: 255
    got = xm.halve(img)
    assert tuple(got[0, 0]) == (1, 1, 1, 1) and tuple(got[1, 1]) == (255,) * 4 and tuple(got[0, 1]) == (0,) * 4


# ---- the mutants: each named case tells its mutant from the model, and the model gives the stated vector at every radius

@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_named_case_tells_its_mutant_from_the_model(name):
    prev, curr, low, (x, y), want, mutant = xc.CASES[name]()
    for radius in RADII:
        got = xm.expand(prev, curr, low, radius)
        assert tuple(int(c) for c in got[y, x]) == want, (name, radius)
        bad = xm.expand(prev, curr, low, radius, mutant=mutant)
        assert tuple(int(c) for c in bad[y, x]) != want, (name, radius, mutant)


def test_every_mutant_has_a_case():
    assert sorted(c()[5] for c in xc.CASES.values()) == sorted(xm.MUTANTS)


# ---- what the route is for: the half-size pyramid's field, expanded, against the full-size pyramid's on synth pans

def psnr(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float((d * d).mean()), 1e-12))


@pytest.fixture(scope="module")
def pan_fields():
    """Per pan and pair: the full-resolution pyramid's field and the expanded half-resolution one at radius 1 and 2."""
    out = {}
    for pan in xc.PANS:
        f0, f1, f2 = xc.pan_frames(pan)
        for pair, (prev, curr) in (("even", (f0, f2)), ("odd", (f0, f1))):
            low = pm.motion_pyramid(xm.halve(prev), xm.halve(curr), 1, 16, 2)
            out[pan, pair] = (prev, curr, f1, pm.motion_pyramid(prev, curr, 2, 16, 2), {r: xm.expand(prev, curr, low, r) for r in (1, 2)})
    return out


def interior(a):
    return a[xc.INTERIOR:-xc.INTERIOR, xc.INTERIOR:-xc.INTERIOR]


@pytest.mark.parametrize("pan", xc.PANS)
@pytest.mark.parametrize("radius", [1, 2])
def test_even_pan_equals_the_full_resolution_pyramid_in_the_interior(pan_fields, pan, radius):
    prev, curr, held_out, full, expanded = pan_fields[pan, "even"]
    assert (interior(full) == (-2 * pan[0], -2 * pan[1])).all()
    assert (interior(expanded[radius]) == interior(full)).all()
    print(f"pan {pan} f0->f2, held-out f1 at t = 0.5: full-resolution pyramid {psnr(mc.interpolate_compensated(prev, curr, full, 0.5), held_out):.2f} dB, "
          f"expanded radius {radius} {psnr(mc.interpolate_compensated(prev, curr, expanded[radius], 0.5), held_out):.2f} dB")


@pytest.mark.parametrize("pan", xc.PANS)
@pytest.mark.parametrize("radius", [1, 2])
def test_odd_pan_agrees_with_the_full_resolution_pyramid_on_99_percent_of_the_interior(pan_fields, pan, radius):
    """The vector (-pan) is odd in at least one component: no doubled vector equals it, the +-1 step recovers it."""
    _, _, _, full, expanded = pan_fields[pan, "odd"]
    agree = float((interior(expanded[radius]) == interior(full)).all(-1).mean())
    print(f"pan {pan} f0->f1 radius {radius}: {100.0 * agree:.2f} % of the interior agrees")
    assert agree >= 0.99
