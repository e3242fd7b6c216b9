"""lfg_interpolate_compensated on the GPU against the CPU model (tests/mc_model.py), byte for byte; what it gets right that
the shader's modes do not; the interpolator switch of lfg_interpolate_frames[_multi]; argument checks; lanes; the host's
--interpolator option; and the hand-made cases of test_mc_model.py that need no hand-placed key image."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import mc_model as mc
from tests.gpu_kit import ctx, first_bad, gpu_vectors, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (33, 17), (64, 64), (257, 131)]
# Dyadic factors make every product of the position arithmetic exact in fp32; the inexact ones are those that tell the model's
# mutants from the model (test_mc_model.py), and the last two approach t = 1 and t = 0 without reaching them.
FACTORS = cases.DYADIC_FACTORS + cases.INEXACT_FACTORS + cases.LIMIT_FACTORS
MATCH = [0, 48, 1020]


def case(ctx, field, w, h, seed):
    """(prev, curr, mv int8) for one kind of vector field: an estimator's on the GPU, or one of cases.field."""
    if field in ("motion", "pyramid"):
        prev = synth.make_prev(w, h, synth.BASE_SEED + seed)
        curr = synth.translate(prev, (5, -3) if field == "motion" else (-30, 18), synth.BASE_SEED + seed)
        return prev, curr, gpu_vectors(ctx, prev, curr, "full" if field == "motion" else "pyramid")
    return cases.field(field, w, h, seed)


def run(ctx, prev, curr, mv, t, match_sad):
    h, w = prev.shape[:2]
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o = ctx.create_frame(w, h)
    try:
        ctx.interpolate_compensated(p, c, m, o, t, match_sad)
        return ctx.download(o)
    finally:
        for f in (p, c, m, o):
            ctx.destroy_frame(f)


@pytest.mark.parametrize("field", ["uniform", "piecewise", "random", "motion", "pyramid"])
def test_every_pixel_equals_the_model(ctx, field):
    for i, (w, h) in enumerate(SIZES):
        prev, curr, mv = case(ctx, field, w, h, 13 * i + 5)
        for t in FACTORS:
            for ms in MATCH:
                got = run(ctx, prev, curr, mv, t, ms)
                want = mc.interpolate_compensated(prev, curr, mv, t, ms)
                assert (got == want).all(), f"{w}x{h} {field} t={t} match_sad={ms}: {first_bad(got, want)}"


@pytest.mark.parametrize("w,h", [(640, 360), (1920, 1080)])
def test_full_frames(ctx, w, h):
    for field in ("piecewise", "random", "motion", "pyramid"):
        prev, curr, mv = case(ctx, field, w, h, 3)
        inexact = list(zip(cases.INEXACT_FACTORS + cases.LIMIT_FACTORS, (1020, 48, 0, 1020, 48, 1020)))
        for t, ms in [(0.25, 48), (0.5, 1020), (0.75, 0)] + inexact:
            got = run(ctx, prev, curr, mv, t, ms)
            want = mc.interpolate_compensated(prev, curr, mv, t, ms)
            assert (got == want).all(), f"{w}x{h} {field} t={t}: {first_bad(got, want)}"


@pytest.mark.parametrize("w,h", [(3840, 2160), (7680, 4320)])
def test_rois_of_4k_and_8k(ctx, w, h):
    rng = np.random.default_rng(w)
    rois = [(0, 0, 64, 64), (w - 64, h - 64, 64, 64)] + [(int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64)), 64, 64)
                                                         for _ in range(6)]
    inexact = [("random", t, 1020) for t in cases.INEXACT_FACTORS + cases.LIMIT_FACTORS] if w == 3840 else []
    for field, t, ms in [("random", 0.5, 1020), ("motion", 0.25, 48)] + inexact:
        prev, curr, mv = case(ctx, field, w, h, 9)
        got = run(ctx, prev, curr, mv, t, ms)
        for x, y, rw, rh in rois:
            want = mc.interpolate_compensated(prev, curr, mv, t, ms, roi=(x, y, rw, rh))
            assert (got[y:y + rh, x:x + rw] == want).all(), (w, h, field, x, y)


def test_padded_pitch(ctx):
    w, h = 257, 131
    prev, curr, mv = case(ctx, "random", w, h, 17)
    bp, p = pitched(ctx, prev, 3)
    bc, c = pitched(ctx, curr, 5)
    bm, m = pitched(ctx, mv, 7, capi.FORMAT_MV_S8X2)
    bo, o = pitched(ctx, np.zeros((h, w, 4), np.uint8), 9)
    try:
        inexact = list(zip(cases.INEXACT_FACTORS + cases.LIMIT_FACTORS, (1020, 0, 48, 1020, 1020, 0)))
        for t, ms in [(0.5, 1020), (0.25, 0)] + inexact:
            ctx.interpolate_compensated(p, c, m, o, t, ms)
            raw = ctx.download(bo)
            assert (raw[:, w:] == 0x5A).all()                     # the padding is not written
            want = mc.interpolate_compensated(prev, curr, mv, t, ms)
            assert (raw[:, :w] == want).all(), first_bad(raw[:, :w], want)
    finally:
        for f in (bp, bc, bm, bo):
            ctx.destroy_frame(f)


def test_multi_equals_single_calls(ctx):
    w, h = 640, 360
    prev, curr, mv = case(ctx, "piecewise", w, h, 23)
    factors = [0.25, 0.5, 0.75, 1.0, 0.0] + cases.INEXACT_FACTORS + cases.LIMIT_FACTORS
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    outs = [ctx.create_frame(w, h) for _ in factors]
    try:
        ctx.interpolate_compensated_multi(p, c, m, outs, factors, 48)
        multi = [ctx.download(o) for o in outs]
        for t, got in zip(factors, multi):
            ctx.interpolate_compensated(p, c, m, outs[0], t, 48)
            assert (got == ctx.download(outs[0])).all(), t
            if t in cases.INEXACT_FACTORS + cases.LIMIT_FACTORS:
                assert (got == mc.interpolate_compensated(prev, curr, mv, t, 48)).all(), t
    finally:
        for f in [p, c, m] + outs:
            ctx.destroy_frame(f)


# ---- the hand-made cases of test_mc_model.py (tests/cases.py), through the GPU call

def test_hand_made_cases(ctx):
    """Each input at every factor equals the model, and at t = 0.5 the literal value that the CPU test states.  The cases on
    flat black frames generate black whatever is projected, so the two that are about the projection alone also run on
    textured frames with match_sad 1020, where the model's key image is the same (asserted here) and shows in the bytes."""
    def check(prev, curr, mv, ms, name):
        outs = {}
        for t in FACTORS:
            outs[t] = run(ctx, prev, curr, mv, t, ms)
            want = mc.interpolate_compensated(prev, curr, mv, t, ms)
            assert (outs[t] == want).all(), f"{name} t={t} match_sad={ms}: {first_bad(outs[t], want)}"
        assert (outs[1.0] == curr).all(), name                         # the header: t = 1 gives curr
        return outs[0.5]

    prev, curr, mv, winners = cases.mc_collision()
    K = mc.keys(prev, curr, mv, 0.5, 0)
    assert all(K[y, x] == mc.key(*v) for (x, y), v in winners.items())
    assert (check(prev, curr, mv, 0, "collision") == 0).all()
    prev, curr, mv, _ = cases.mc_collision(textured_frames=True)
    assert (mc.keys(prev, curr, mv, 0.5, 1020) == K).all()
    got = check(prev, curr, mv, 1020, "collision, textured")
    for (x, y), v in winners.items():                                # the winner's vector, not a loser's, samples the pixel
        K1 = np.full((8, 8), mc.key(*v), np.uint32)
        assert (got[y, x] == mc.sample(prev, curr, mv, K1, 0.5, 1020)[y, x]).all(), (x, y)

    prev, curr, mv = cases.mc_unmatched_source()
    for ms in (199, 200):
        check(prev, curr, mv, ms, "unmatched source")

    prev, curr, mv = cases.mc_projection_outside()
    assert (check(prev, curr, mv, 0, "projection outside") == 0).all()
    prev, curr, mv = cases.mc_projection_outside(textured_frames=True)
    assert (mc.keys(prev, curr, mv, 0.5, 1020) == mc.keys(*cases.mc_projection_outside(), 0.5, 0)).all()
    check(prev, curr, mv, 1020, "projection outside, textured")

    prev, curr, mv, obj = cases.mc_revealed_and_covered()
    got = check(prev, curr, mv, 0, "revealed and covered")
    assert (got[2, 5] == obj).all()                                   # half way
    assert (got[2, 4] == curr[2, 4]).all() and (got[2, 6] == prev[2, 6]).all()
    want = np.zeros_like(prev)
    want[2, 5] = obj
    assert (got == want).all()

    prev, curr, mv = cases.mc_row_projected_to_the_top()
    got = check(prev, curr, mv, 1020, "row projected to the top")
    assert (got[1] == curr[3]).all()

    for w, h, seed in ((1, 1, 1), (7, 5, 2), (50, 40, 3)):           # t = 1 gives curr for any vectors and match_sad
        prev, curr = cases.textured(w, h, seed), cases.textured(w, h, seed + 100)
        mv = np.random.default_rng(seed).integers(-128, 128, (h, w, 2)).astype(np.int8)
        for ms in (0, 48, 1020):
            assert (run(ctx, prev, curr, mv, 1.0, ms) == curr).all(), (w, h, ms)


def test_the_walk_reaches_16(ctx):
    """cases.mc_walk_reach: one projected pixel in a key image of holes.  Byte for byte the model, and literally: the holes at
    distance 16 along an axis are filled from it, those at 17 are not."""
    prev, curr, mv, blank = cases.mc_walk_reach()
    ms = cases.WALK_REACH_MATCH_SAD
    for t in cases.WALK_REACH_FACTORS:
        got, got_blank = run(ctx, prev, curr, mv, t, ms), run(ctx, prev, curr, blank, t, ms)
        for g, field in ((got, mv), (got_blank, blank)):
            want = mc.interpolate_compensated(prev, curr, field, t, ms)
            assert (g == want).all(), f"t={t}: {first_bad(g, want)}"
        cases.check_walk_reach(got, got_blank, t)


# ---- what the shader's modes do not do: content at time t where it is

def test_4k_pan_full_search(ctx):
    w, h = 3840, 2160
    prev = synth.make_prev(w, h)
    curr = synth.translate(prev, (6, -4))
    mv = gpu_vectors(ctx, prev, curr, "full")
    got = run(ctx, prev, curr, mv, 0.5, 48)
    want = synth.translate(prev, (3, -2))
    assert (got[24:-24, 24:-24] == want[24:-24, 24:-24]).all(), first_bad(got[24:-24, 24:-24], want[24:-24, 24:-24])


def test_4k_pan_pyramid(ctx):
    w, h = 3840, 2160
    prev = synth.make_prev(w, h)
    curr = synth.translate(prev, (40, -24))
    mv = gpu_vectors(ctx, prev, curr, "pyramid")
    got = run(ctx, prev, curr, mv, 0.5, 48)
    want = synth.translate(prev, (20, -12))
    assert (got[100:-100, 100:-100] == want[100:-100, 100:-100]).all(), first_bad(got[100:-100, 100:-100], want[100:-100, 100:-100])


def test_moving_square(ctx):
    prev, curr, (x, y) = mc.moving_square()
    mv = gpu_vectors(ctx, prev, curr, "full")
    bg = np.random.default_rng(7).integers(0, 256, prev.shape, dtype=np.uint8)     # moving_square's own background
    for t in (0.25, 0.5, 0.75):
        s = int(12 * t)
        truth = bg.copy()
        truth[y:y + 16, x + s:x + s + 16] = prev[y:y + 16, x:x + 16]
        got = run(ctx, prev, curr, mv, t, 48)
        assert (got == mc.interpolate_compensated(prev, curr, mv, t, 48)).all()
        ok = (got == truth).all(-1)
        assert ok[y + 4:y + 12, x + s + 4:x + s + 12].all(), t
        swept = np.zeros_like(ok)
        swept[y - 4:y + 20, x - 4:x + 12 + 20] = True
        assert ok[~swept].all(), t


# ---- the interpolator switch

@pytest.mark.parametrize("estimator", [capi.ESTIMATOR_FULL_SEARCH, capi.ESTIMATOR_PYRAMID])
def test_interpolator_switch(ctx, estimator):
    w, h = 640, 360
    prev = synth.make_prev(w, h)
    curr = synth.translate(prev, (9, -5))
    factors = [0.25, 0.5, 0.75]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    outs = [ctx.create_frame(w, h) for _ in factors]
    ref = ctx.create_frame(w, h)
    try:
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        ctx.set_motion_estimator(estimator)
        if estimator == capi.ESTIMATOR_PYRAMID:
            ctx.motion_pyramid(p, c, m, 2, 16, 2)
        else:
            ctx.motion(p, c, m)
        for ms in (48, 300):
            want = {}
            for t in factors:
                ctx.interpolate_compensated(p, c, m, ref, t, ms)
                want[t] = ctx.download(ref)
            ctx.set_interpolator(capi.INTERPOLATOR_COMPENSATED, ms)
            for fused in (False, True):
                ctx.set_fused_motion_interpolate(fused)
                ctx.interpolate_frames(p, c, outs[0], 0.5)
                assert (ctx.download(outs[0]) == want[0.5]).all(), (ms, fused)
                ctx.interpolate_frames_multi(p, c, outs, factors)
                for t, o in zip(factors, outs):
                    assert (ctx.download(o) == want[t]).all(), (ms, fused, t)
            ctx.set_fused_motion_interpolate(False)
        # back on the shader: lfg_motion (or the pyramid) followed by lfg_interpolate
        ctx.set_interpolator(capi.INTERPOLATOR_SHADER)
        ctx.interpolate_frames(p, c, outs[0], 0.5)
        ctx.interpolate(p, c, m, ref, 0.5)
        assert (ctx.download(outs[0]) == ctx.download(ref)).all()
    finally:
        ctx.set_interpolator(capi.INTERPOLATOR_SHADER)
        ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
        ctx.set_semantics(capi.SEMANTICS_REFERENCE)
        ctx.set_fused_motion_interpolate(False)
        for f in [p, c, m, ref] + outs:
            ctx.destroy_frame(f)


def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 40, 24
    prev, curr, mv = case(ctx, "random", w, h, 1)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o, o2 = ctx.create_frame(w, h), ctx.create_frame(w, h)
    pattern = np.full((h, w, 4), 0x5A, np.uint8)
    ctx.upload(o, pattern)
    ctx.upload(o2, pattern)
    small = ctx.create_frame(w - 1, h)
    small_mv = ctx.create_frame(w, h - 1, capi.FORMAT_MV_S8X2)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)    # a pitch that is not a multiple of 4
    big = ctx.create_frame(w, h)
    mv_in_big = capi.Context.wrap(big.data, w, h, capi.FORMAT_MV_S8X2, pitch=w * 2)  # vectors in the first half of `big`
    empty = capi.Frame()
    B = ctypes.byref

    def single(a, b, v, out, t=0.5, ms=48):
        return lib.lfg_interpolate_compensated(ctx.h, a and B(a), b and B(b), v and B(v), out and B(out), t, ms)

    bad = [
        single(None, c, m, o), single(p, c, None, o), single(p, c, m, None), single(empty, c, m, o),
        single(p, c, p, o),                      # mv of the wrong format
        single(p, m, m, o),                      # curr of the wrong format
        single(p, c, m, small), single(p, c, small_mv, o),
        single(odd, c, m, o), single(p, odd, m, o),
        single(p, c, m, p), single(p, c, m, c), single(p, c, mv_in_big, big),       # the output overlaps an input
        single(p, c, m, o, float("nan")), single(p, c, m, o, float("inf")), single(p, c, m, o, -0.01), single(p, c, m, o, 1.01),
        single(p, c, m, o, 0.5, -1), single(p, c, m, o, 0.5, 1021),
    ]

    def multi(outs, factors, count=None, ms=48):
        po = (capi._FP * len(outs))(*[ctypes.pointer(f) for f in outs])
        pf = (ctypes.c_float * len(factors))(*factors)
        return lib.lfg_interpolate_compensated_multi(ctx.h, B(p), B(c), B(m), po, pf, len(outs) if count is None else count, ms)

    bad += [
        multi([o, o], [0.25, 0.5]),              # two outputs alias each other
        multi([o], [0.5], count=0), multi([o] * 17, [0.5] * 17),
        multi([o, o2], [0.5, float("nan")]), multi([o, o2], [0.5, 0.5], ms=2000),
        multi([o, c], [0.5, 0.5]),
    ]
    assert all(rc == -1 for rc in bad), bad                          # LFG_ERR_INVALID
    assert lib.lfg_set_interpolator(ctx.h, 2, 48) == -1
    assert lib.lfg_set_interpolator(ctx.h, 1, 1021) == -1
    assert lib.lfg_set_interpolator(ctx.h, 1, -1) == -1
    assert lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert (ctx.download(o) == pattern).all() and (ctx.download(o2) == pattern).all()
    # the shader path is still the default: lfg_interpolate_frames after the failed settings equals motion + interpolate
    ref = ctx.create_frame(w, h)
    ctx.interpolate_frames(p, c, o, 0.5)
    ctx.motion(p, c, m)
    ctx.interpolate(p, c, m, ref, 0.5)
    assert (ctx.download(o) == ctx.download(ref)).all()
    for f in (p, c, m, o, o2, small, small_mv, wide, big, ref):
        ctx.destroy_frame(f)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (96, 64), (200, 120), (130, 90), (96, 64), (300, 170)]
    cases = [case(ctx, "random" if i % 2 else "piecewise", w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    alone = [run(ctx, a, b, v, 0.5, 1020) for a, b, v in cases]

    def enqueue(i, a, b, v):
        h, w = a.shape[:2]
        p, c, m = ctx.frame_from(a), ctx.frame_from(b), ctx.frame_from(v, capi.FORMAT_MV_S8X2)
        o = ctx.create_frame(w, h)
        ctx.interpolate_compensated(p, c, m, o, 0.5, 1020)
        return p, c, m, o

    three_lanes(ctx, cases, enqueue, alone)


def test_host_compensated_stream_matches_capi(tmp_path):
    w, h, n = 1920, 1080, 3
    frames = [synth.make_prev(w, h)]
    for k in range(1, n):
        frames.append(synth.translate(frames[-1], (12, -6), synth.BASE_SEED + k))
    _, got = host_run(tmp_path, frames, (w, h), "--semantics", "intended", "--interpolator", "compensated")
    assert len(got) == 2 * n - 1
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ins = [c.frame_from(f) for f in frames]
        ups = [c.create_frame(w, h) for _ in frames]
        for i, u in zip(ins, ups):
            c.scale(i, u)
        m = c.create_frame(w, h, capi.FORMAT_MV_S8X2)
        o = c.create_frame(w, h)
        want = [c.download(ups[0])]
        for k in range(1, n):
            c.motion(ups[k - 1], ups[k], m)
            c.interpolate_compensated(ups[k - 1], ups[k], m, o, 0.5, 48)
            want += [c.download(o), c.download(ups[k])]
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k
