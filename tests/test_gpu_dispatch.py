"""The dispatch of lfg_interpolate_frames and lfg_interpolate_frames_multi against the CPU chain (tests/cases.py: the
estimator's model, then the refine model when the radius is >= 0, then the interpolation model), byte for byte on every pixel:
every combination of estimator, refinement radius, interpolator, semantics and fused-motion flag; settings changed between
enqueued calls; frame sizes that change under the per-lane temporaries; three lanes; and a default that never moved."""
import numpy as np
import pytest

from linux_fg_amd import capi
from tests import cases
from tests.gpu_kit import DEFAULT, apply, ctx, first_bad

pytestmark = pytest.mark.gpu


def restore(ctx):
    ctx.lane_select(0)
    ctx.lanes(1)
    apply(ctx, DEFAULT)


_chains = {}


def chain_of(key, make):
    """One cases.Chain per input pair for the whole module: the estimators' models run once per pair."""
    if key not in _chains:
        _chains[key] = cases.Chain(*make())
    return _chains[key]


# ---- 1. the full matrix on one scene

@pytest.fixture(scope="module")
def matrix(ctx):
    ch = chain_of("matrix", cases.matrix_scene)
    h, w = ch.prev.shape[:2]
    p, c = ctx.frame_from(ch.prev), ctx.frame_from(ch.curr)
    outs = [ctx.create_frame(w, h) for _ in range(1 + len(cases.MATRIX_FACTORS))]
    yield ch, p, c, outs
    for f in [p, c] + outs:
        ctx.destroy_frame(f)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("setting", cases.SETTINGS, ids=lambda s: "-".join(str(v) for v in s))
def test_every_setting_equals_the_chain(ctx, matrix, setting, fused):
    """64 settings x both entry points.  The scene tells any two settings apart that the header defines differently
    (test_mc_model.py: test_matrix_scene_tells_the_settings_apart), so a branch that runs another setting's stages fails."""
    ch, p, c, outs = matrix
    try:
        apply(ctx, setting, fused)
        ctx.interpolate_frames(p, c, outs[0], cases.MATRIX_FACTOR)
        ctx.interpolate_frames_multi(p, c, outs[1:], cases.MATRIX_FACTORS)
        got = [ctx.download(o) for o in outs]
    finally:
        restore(ctx)
    want = ch.frames(setting, [cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS)
    for t, g, e in zip([cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS, got, want):
        assert (g == e).all(), f"{setting} fused={fused} t={t}: {first_bad(g, e)}"


# ---- 2. settings changed between enqueued calls

# (setting, match_sad, factor); the fused flag alternates
SEQUENCE = [
    (("full", -1, "shader", 0), 48, 0.3),
    (("pyramid", 2, "compensated", 1), 300, 0.9),
    (("full", 1, "shader", 0), 48, 0.5),
    (("full", -1, "compensated", 0), 0, 5.0 / 6.0),
    (("pyramid", -1, "shader", 1), 48, 0.7),
    (("full", 0, "compensated", 1), 1020, 0.3),
    (("pyramid", 0, "shader", 0), 48, 0.25),
    (("full", 2, "shader", 1), 48, 0.9),
    (("pyramid", 1, "compensated", 0), 48, 0.3),
    (("full", -1, "compensated", 1), 48, 0.3),
    (("full", -1, "shader", 1), 48, 0.7),
]


def test_settings_changed_between_enqueued_calls(ctx, matrix):
    """One context, the setters between the calls, one sync at the end: output k is the chain under the settings in force
    when call k was made.  Twice: in the second round every temporary exists, so the library has no reason to wait either."""
    ch, p, c, _ = matrix
    h, w = ch.prev.shape[:2]
    want = [ch.frames(s, [t], ms)[0] for s, ms, t in SEQUENCE]
    assert len({e.tobytes() for e in want}) == len(SEQUENCE)         # a call that ran under a neighbour's settings shows
    for (s, ms, t), e in zip(SEQUENCE, want):                        # and so does one that kept the default match_sad
        assert ms == capi.DEFAULT_MATCH_SAD or (e != ch.frames(s, [t], capi.DEFAULT_MATCH_SAD)[0]).any(), (s, ms, t)
    outs = [ctx.create_frame(w, h) for _ in SEQUENCE]
    try:
        for rnd in range(2):
            for o in outs:
                ctx.upload(o, np.full((h, w, 4), 0x5A, np.uint8))
            for k, ((s, ms, t), o) in enumerate(zip(SEQUENCE, outs)):
                apply(ctx, s, fused=k % 2 == 1, match_sad=ms)
                ctx.interpolate_frames(p, c, o, t)
            ctx.sync()
            for k, (o, e) in enumerate(zip(outs, want)):
                g = ctx.download(o)
                assert (g == e).all(), f"round {rnd} call {k} {SEQUENCE[k]}: {first_bad(g, e)}"
    finally:
        restore(ctx)
        for o in outs:
            ctx.destroy_frame(o)


# ---- 3. and 4. sizes that change under the temporaries, on one lane and on three

# large, small, large, odd, one pixel: a grown mc_keys reused for a smaller frame, mv_tmp / mv_refined made again, the pyramid
# workspace laid out again; then the same once more in another order.  The scenes (cases.small_scene) are not held to tell
# every setting apart, and the smallest are a bare pan: which branch runs is the matrix's business above, these are about what
# the temporaries hold.
SIZES = [(257, 131), (64, 36), (257, 131), (33, 17), (1, 1), (130, 90), (7, 5), (257, 131), (64, 36)]
SINGLE, MULTI = 0.3, [0.9, 0.25, 5.0 / 6.0]


def run_sequence(ctx, sizes, setting, lanes):
    """Pair k of its own size and content on lane k % lanes, its own buffers, both entry points; everything is enqueued
    before the one sync.  Returns [(chain, [frame at SINGLE] + [frames at MULTI])]."""
    chains = [chain_of(("small", w, h, k), lambda w=w, h=h, k=k: cases.small_scene(w, h, 70 + k)) for k, (w, h) in enumerate(sizes)]
    frames = []
    try:
        for ch in chains:
            h, w = ch.prev.shape[:2]
            frames.append((ctx.frame_from(ch.prev), ctx.frame_from(ch.curr), [ctx.create_frame(w, h) for _ in range(1 + len(MULTI))]))
        ctx.lanes(lanes)
        apply(ctx, setting)
        for k, (p, c, outs) in enumerate(frames):
            ctx.lane_select(k % lanes)
            ctx.interpolate_frames(p, c, outs[0], SINGLE)
            ctx.interpolate_frames_multi(p, c, outs[1:], MULTI)
        ctx.sync()
        return [(ch, [ctx.download(o) for o in outs]) for ch, (_, _, outs) in zip(chains, frames)]
    finally:
        restore(ctx)
        for p, c, outs in frames:
            for f in [p, c] + outs:
                ctx.destroy_frame(f)


def check_sequence(ctx, sizes, setting, lanes):
    for k, (ch, got) in enumerate(run_sequence(ctx, sizes, setting, lanes)):
        want = ch.frames(setting, [SINGLE] + MULTI)
        for t, g, e in zip([SINGLE] + MULTI, got, want):
            assert (g == e).all(), f"{setting} lanes={lanes} pair {k} {sizes[k]} t={t}: {first_bad(g, e)}"


@pytest.mark.parametrize("setting", [("pyramid", 1, "compensated", 1), ("pyramid", 2, "compensated", 0), ("full", 0, "shader", 1)],
                         ids=lambda s: "-".join(str(v) for v in s))
def test_sizes_that_change_under_the_temporaries(ctx, setting):
    check_sequence(ctx, SIZES[:5], setting, 1)


LANE_SETTINGS = [("full", -1, "compensated", 1), ("pyramid", 2, "compensated", 1), ("pyramid", 0, "shader", 1),
                 ("full", 1, "shader", 0)]


@pytest.mark.parametrize("setting", LANE_SETTINGS, ids=lambda s: "-".join(str(v) for v in s))
def test_three_lanes_equal_the_chain(ctx, setting):
    """Frames in flight on three lanes, each lane's temporaries changing size from call to call: every output is the chain,
    which the one-lane run (the same sequence, run first) equals too."""
    check_sequence(ctx, SIZES, setting, 1)
    check_sequence(ctx, SIZES, setting, 3)


# ---- 5. a default that never moved

def test_restored_context_equals_a_fresh_one(ctx, matrix):
    """Last in the file: the context that went through every setting above -- and, so that it holds when run alone, through
    the opt-in stages once more here -- with every setter put back, against a context that touched no setter at all, and
    both against the chain of the default setting."""
    ch, p, c, outs = matrix
    try:
        for k, s in enumerate((("pyramid", 2, "compensated", 1), ("full", 0, "shader", 1), ("full", -1, "compensated", 0))):
            apply(ctx, s, fused=k % 2 == 0, match_sad=300)
            ctx.interpolate_frames(p, c, outs[0], 0.7)
            ctx.interpolate_frames_multi(p, c, outs[1:], cases.MATRIX_FACTORS)
    finally:
        restore(ctx)
    factors = [cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS
    used = []
    for t, o in zip(factors, outs):
        ctx.interpolate_frames(p, c, o, t)
        used.append(ctx.download(o))
    h, w = ch.prev.shape[:2]
    with capi.Context(0) as fresh:
        fp, fc, fo = fresh.frame_from(ch.prev), fresh.frame_from(ch.curr), fresh.create_frame(w, h)
        for t, u, e in zip(factors, used, ch.frames(DEFAULT, factors)):
            fresh.interpolate_frames(fp, fc, fo, t)
            g = fresh.download(fo)
            assert (u == g).all(), f"t={t}: the used context differs from a fresh one: {first_bad(u, g)}"
            assert (g == e).all(), f"t={t}: {first_bad(g, e)}"
