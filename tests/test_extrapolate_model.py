"""The CPU model of lfg_extrapolate_compensated (tests/extrapolate_model.py) against the header's own statements: the three
"Hence" properties, a held-out pan, the moving square with its donor rule, the mutants of extrapolate_model.c and the power of
the shared cases (tests/extrapolate_cases.py) that the GPU test runs byte for byte."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import cases
from tests import extrapolate_cases as xc
from tests import extrapolate_model as ex
from tests import mc_model as mc


# ---- the header's "Hence"

@pytest.mark.parametrize("ms", xc.MATCH)
def test_zero_ahead_gives_curr(ms):
    for w, h, seed in ((1, 1, 1), (7, 5, 2), (50, 40, 3)):
        prev, curr = cases.textured(w, h, seed), cases.textured(w, h, seed + 100)
        mv = np.random.default_rng(seed).integers(-128, 128, (h, w, 2)).astype(np.int8)
        assert (ex.extrapolate(prev, curr, mv, 0.0, ms) == curr).all(), (w, h)
        prev, curr, mv = cases.field("piecewise", w, h, seed)            # a field most of whose pixels do match
        assert (ex.extrapolate(prev, curr, mv, 0.0, ms) == curr).all(), (w, h)


def _shifted_equal(out, curr, v):
    """out(d) == curr(d + v) at every d whose source d + v lies inside the image."""
    h, w = curr.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs + v[0], ys + v[1]
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    assert inside.any()
    return (out[inside] == curr[sy[inside], sx[inside]]).all()


@pytest.mark.parametrize("ms", xc.MATCH)
def test_uniform_vector_shifts_curr(ms):
    """curr(q) = prev(q + v), 0 where q + v leaves the image (the gate's own reading of prev there): v matches everywhere,
    even at match_sad 0."""
    rng = np.random.default_rng(11 + ms)
    for w, h in ((40, 24), (7, 5)):
        for _ in range(6):
            v = rng.integers(-1, 2, 2) * 2 if w == 7 else rng.integers(-9, 10, 2) * 2       # even, so v / 2 is whole
            mv = np.broadcast_to(v.astype(np.int8), (h, w, 2))
            prev = cases.textured(w, h, int(rng.integers(1 << 30)))
            curr = cases.warp(prev, mv)
            assert (ex.keys(prev, curr, mv, 1.0, ms) != ex.HOLE).sum() > 0
            assert _shifted_equal(ex.extrapolate(prev, curr, mv, 1.0, ms), curr, v), (w, h, v)
            assert _shifted_equal(ex.extrapolate(prev, curr, mv, 0.5, ms), curr, v // 2), (w, h, v)
        odd = np.array([3, -1])                                                           # a = 1 needs no even vector
        mv = np.broadcast_to(odd.astype(np.int8), (h, w, 2))
        prev = cases.textured(w, h, 99)
        assert _shifted_equal(ex.extrapolate(prev, cases.warp(prev, mv), mv, 1.0, ms), cases.warp(prev, mv), odd)


# ---- a held-out pan: frames 0 and 1 predict frame 2

PAN = (3, -2)
# A block's vector is wrong where its 8 x 8 block or its search window (radius 16) reaches content that entered the frame, and
# a pixel within the pan's largest component of the edge has no source in frame 1: 16 + 4 + 3 px, and no more than 32.
BORDER = 16 + 4 + max(abs(PAN[0]), abs(PAN[1]))


def pan_frames(w, h):
    f0 = synth.make_prev(w, h)
    f1 = synth.translate(f0, PAN, synth.BASE_SEED + 1)
    return f0, f1, synth.translate(f1, PAN, synth.BASE_SEED + 2)


@pytest.mark.parametrize("w,h", [(96, 64), (200, 120)])
def test_held_out_pan(w, h):
    import oracle
    assert BORDER <= 32
    f0, f1, f2 = pan_frames(w, h)
    mv = oracle.motion(f0, f1, semantics=1).astype(np.int8)
    out = ex.extrapolate(f0, f1, mv, 1.0)
    b = BORDER
    assert (out[b:-b, b:-b] == f2[b:-b, b:-b]).all()
    wrong, repeated = int((out != f2).any(-1).sum()), int((f1 != f2).any(-1).sum())
    print(f"{w}x{h}: extrapolation differs from frame 2 in {wrong} pixels, repeating frame 1 in {repeated}")
    assert wrong < repeated


# ---- the moving square: where the square is, what the revealed strip shows, and the donor rule

@pytest.mark.parametrize("a", [0.5, 1.0])
def test_moving_square(a):
    """mc_model.moving_square with its true per-pixel vectors: the square's pixels hold (-12, 0), the background (0, 0).  The
    strip that the square left between prev and curr (12 px wide) does not match under (0, 0) and is a hole; the strip that it
    vacates after curr (12 a px wide) is a hole whose c holds the square: the donor branch, 12 a * 16 pixels of it."""
    size, shift = 16, (12, 0)
    prev, curr, (x, y) = mc.moving_square(size=size, shift=shift)
    cx = x + shift[0]                                                   # the square's left edge in curr
    mv = np.zeros(prev.shape[:2] + (2,), np.int8)
    mv[y:y + size, cx:cx + size] = (-shift[0], -shift[1])
    out = ex.extrapolate(prev, curr, mv, a)
    how = ex.branches(prev, curr, mv, a)
    s = int(shift[0] * a)
    assert (out[y:y + size, cx + s:cx + s + size] == curr[y:y + size, cx:cx + size]).all()          # the square, moved on
    bg = np.random.default_rng(7).integers(0, 256, prev.shape, dtype=np.uint8)                      # moving_square's background
    assert (curr[y:y + size, x:cx] == bg[y:y + size, x:cx]).all()
    assert (out[y:y + size, x:cx] == curr[y:y + size, x:cx]).all()                                  # revealed: curr's background
    vacated = (slice(y, y + size), slice(cx, cx + s))
    assert not (out[vacated] == curr[vacated]).all(-1).any()            # no copy of the square is left behind it
    taken = int((how == ex.DONOR_TAKEN).sum())
    assert taken == s * size and taken > 0
    assert (how[vacated] == ex.DONOR_TAKEN).all()
    outside = np.ones(how.shape, bool)
    outside[y:y + size, x:cx + s + size] = False
    assert (out[outside] == curr[outside]).all()                        # the static background stays


# ---- the mutants of extrapolate_model.c: which shared case, at which factor, tells each from the model

TELLS = {
    "PLUS_V": ("uniform 33x17 match_sad=1020", 1.0),
    "CEIL_PROJECT": ("random 33x17 match_sad=1020", 0.5),
    "ONE_MINUS_A": ("uniform 33x17 match_sad=1020", 0.25),
    "NO_DONOR": ("moving square", 1.0),
    "LATER_TIE": ("tie, collision, foreground", 1.0),
}


@pytest.fixture(scope="module")
def shared():
    return {name: rest for name, *rest in xc.shared_cases()}


@pytest.mark.parametrize("mutant", ex.MUTANTS)
def test_shared_cases_tell_the_mutants_from_the_model(shared, mutant):
    name, a = TELLS[mutant]
    assert a in xc.FACTORS
    prev, curr, mv, ms = shared[name]
    assert (ex.extrapolate(prev, curr, mv, a, ms, mutant=mutant) != ex.extrapolate(prev, curr, mv, a, ms)).any(), (mutant, name, a)


def test_mutants_agree_where_they_must(shared):
    """The rewrites are no strawmen: at a = 0 every one of them gives curr, as the model does."""
    prev, curr, mv, ms = shared["piecewise 33x17 match_sad=48"]
    for mutant in ex.MUTANTS:
        if mutant != "ONE_MINUS_A":
            assert (ex.extrapolate(prev, curr, mv, 0.0, ms, mutant=mutant) == curr).all(), mutant
    assert (ex.extrapolate(prev, curr, mv, 0.5, ms, mutant="ONE_MINUS_A") == ex.extrapolate(prev, curr, mv, 0.5, ms)).all()


# ---- the power of the shared cases

KINDS = ("colliding projections", "holes with no donor", "equal triple from two directions", "holes at the image edge",
         "samples clamped outside the image", "donor branch taken")


def test_shared_cases_hold_every_kind(shared):
    found = {}
    for name, (prev, curr, mv, ms) in shared.items():
        for a in xc.FACTORS:
            for kind in xc.kinds(prev, curr, mv, a, ms):
                found.setdefault(kind, (name, a))
    for kind in KINDS:
        assert kind in found, f"no shared case has {kind}"
    print(found)


def test_tie_case_reads_as_its_docstring_says():
    prev, curr, mv = xc.tie_collision_foreground()
    K = ex.keys(prev, curr, mv, 1.0, 1020)
    assert (K[3, 6:9] == ex.HOLE).all() and (K[1, 6:9] == ex.key(0, 2)).all() and (K != ex.HOLE).sum() == K.size - 3
    kept = xc.walk(K, 7, 3)
    assert [t for _, t, _ in kept] == [(0, 0, 0)] * 4 and kept[0][2] == (9, 3) and kept[1][2] == (5, 3)
    out = ex.extrapolate(prev, curr, mv, 1.0, 1020)
    assert (out[3, 7] == curr[3, 9]).all() and (out[3, 6] == curr[3, 9]).all() and (out[3, 8] == curr[3, 9]).all()
    assert (out[1, 6:9] == curr[3, 6:9]).all()                          # the colliding destination shows the moved pixels
    assert (ex.branches(prev, curr, mv, 1.0, 1020)[3, 6:9] == ex.DONOR_TAKEN).all()
