"""lfg_motion_refine on the GPU against the CPU model (tests/refine_model.py), byte for byte; argument checks; lanes; the
refinement switch of lfg_interpolate_frames[_multi]; the host's --refine-vectors; the hand-made cases of
test_refine_model.py; and what it is for: the halo of wrong vectors around moving edges."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import mc_model as mc
from tests import pyramid_model as pm
from tests import refine_model as rm
from tests.gpu_kit import ctx, first_bad, gpu_vectors, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (33, 17), (64, 64), (257, 131), (1920, 1080)]
RADII = [0, 1, 2]
FIELDS = ["uniform", "piecewise", "random", "full", "pyramid"]


def case(ctx, field, w, h, seed):
    """(prev, curr, mv int8) for one kind of vector field (the fields of test_gpu_compensated.case, and both estimators)."""
    rng = np.random.default_rng(seed)
    if field in ("full", "pyramid"):
        prev = synth.make_prev(w, h, synth.BASE_SEED + seed)
        curr = synth.translate(prev, (5, -3) if field == "full" else (-30, 18), synth.BASE_SEED + seed)
        return prev, curr, gpu_vectors(ctx, prev, curr, field)
    prev = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    mv = np.zeros((h, w, 2), np.int8)
    if field == "uniform":
        mv[...] = rng.integers(-20, 21, 2)
        curr = synth.translate(prev, tuple(-int(v) for v in mv[0, 0]), synth.BASE_SEED + seed)
    elif field == "piecewise":            # four quadrants with their own vectors
        vs = rng.integers(-12, 13, (4, 2))
        mv[: h // 2, : w // 2], mv[: h // 2, w // 2:], mv[h // 2:, : w // 2], mv[h // 2:, w // 2:] = vs
        curr = np.clip(prev.astype(np.int16) + rng.integers(-6, 7, prev.shape), 0, 255).astype(np.uint8)
    else:                                 # dense random over the full byte range
        mv = rng.integers(-128, 128, (h, w, 2)).astype(np.int8)
        curr = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return prev, curr, mv


def run(ctx, prev, curr, mv, radius):
    h, w = prev.shape[:2]
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        ctx.motion_refine(p, c, m, o, radius)
        return ctx.download(o)
    finally:
        for f in (p, c, m, o):
            ctx.destroy_frame(f)


@pytest.mark.parametrize("field", FIELDS)
def test_every_vector_equals_the_model(ctx, field):
    for i, (w, h) in enumerate(SIZES):
        prev, curr, mv = case(ctx, field, w, h, 13 * i + 5)
        for radius in RADII:
            got = run(ctx, prev, curr, mv, radius)
            want = rm.refine(prev, curr, mv, radius)
            assert (got == want).all(), f"{w}x{h} {field} radius={radius}: {first_bad(got, want)}"
            if field == "uniform":
                assert (got == mv).all()


# ---- the hand-made cases of test_refine_model.py (tests/cases.py), through the GPU call: the model, and the literal value
# that the CPU test states

def vec(a, x, y):
    return tuple(int(c) for c in a[y, x])


@pytest.mark.parametrize("radius", RADII)
def test_hand_made_cases(ctx, radius):
    def check(prev, curr, mv, name):
        got = run(ctx, prev, curr, mv, radius)
        want = rm.refine(prev, curr, mv, radius)
        assert (got == want).all(), f"{name} radius={radius}: {first_bad(got, want)}"
        return got

    for vectors, want in cases.REFINE_TIES:                       # all-zero frames: every cost ties
        got = check(*cases.refine_tie_case(vectors), f"tie {vectors}")
        assert vec(got, 8, 8) == want, vectors
    got = check(*cases.refine_candidates_outside(), "candidates outside")     # 4 x 1: the neighbours lie outside
    assert vec(got, 0, 0) == (2, 0) and vec(got, 1, 0) == (0, 0) and vec(got, 3, 0) == (0, 0)
    got = check(*cases.refine_prev_outside_zero(), "prev outside reads 0")
    for x, y in ((6, 6), (2, 6), (10, 6), (6, 2), (2, 2), (6, 10)):
        assert vec(got, x, y) == (100, 0), (x, y)
    assert vec(got, 0, 0) == (0, 0)
    if radius >= 1:
        for vertical in (True, False):
            prev, curr, mv, truth = cases.refine_straight_edge(radius, vertical)
            got = check(prev, curr, mv, f"straight edge vertical={vertical}")
            assert (got == truth).all(), first_bad(got, truth)
    if radius == 1:
        got = check(*cases.refine_cost_before_length(), "cost before length")
        assert vec(got, 12, 8) == (6, 2) and vec(got, 8, 8) == (6, 2) and vec(got, 16, 8) == (6, 2) and vec(got, 0, 0) == (0, 0)
    prev, curr = cases.textured(1, 1, 50), cases.textured(1, 1, 51)
    for v in ((0, 0), (-128, 127), (3, -7)):                      # a 1 x 1 frame keeps its vector
        assert vec(check(prev, curr, np.array([[v]], np.int8), "1 x 1"), 0, 0) == v


@pytest.mark.parametrize("w,h", [(3840, 2160), (7680, 4320)])
def test_rois_of_4k_and_8k(ctx, w, h):
    rng = np.random.default_rng(w)
    rois = [(0, 0, 64, 64), (w - 64, 0, 64, 64), (0, h - 64, 64, 64), (w - 64, h - 64, 64, 64)] + \
           [(int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64)), 64, 64) for _ in range(4)]
    for field in FIELDS:
        prev, curr, mv = case(ctx, field, w, h, 9)
        for radius in RADII:
            got = run(ctx, prev, curr, mv, radius)
            for x, y, rw, rh in rois:
                want = rm.refine(prev, curr, mv, radius, roi=(x, y, rw, rh))
                assert (got[y:y + rh, x:x + rw] == want).all(), (w, h, field, radius, x, y)


def test_padded_pitch(ctx):
    w, h = 257, 131
    prev, curr, mv = case(ctx, "random", w, h, 17)
    bp, p = pitched(ctx, prev, 3)
    bc, c = pitched(ctx, curr, 5)
    bm, m = pitched(ctx, mv, 7, capi.FORMAT_MV_S8X2)
    bo, o = pitched(ctx, np.zeros((h, w, 2), np.int8), 9, capi.FORMAT_MV_S8X2)
    try:
        for radius in RADII:
            ctx.motion_refine(p, c, m, o, radius)
            raw = ctx.download(bo)
            assert (raw[:, w:].view(np.uint8) == 0x5A).all()          # the padding is not written
            want = rm.refine(prev, curr, mv, radius)
            assert (raw[:, :w] == want).all(), first_bad(raw[:, :w], want)
    finally:
        for f in (bp, bc, bm, bo):
            ctx.destroy_frame(f)


def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 40, 24
    prev, curr, mv = case(ctx, "random", w, h, 1)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    pattern = np.full((h, w, 2), 0x5A, np.int8)
    ctx.upload(o, pattern)
    small = ctx.create_frame(w - 1, h)
    small_mv = ctx.create_frame(w, h - 1, capi.FORMAT_MV_S8X2)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)              # pitch not a multiple of 4
    wide_mv = ctx.create_frame(w + 1, h, capi.FORMAT_MV_S8X2)
    odd_mv = capi.Context.wrap(wide_mv.data, w, h, capi.FORMAT_MV_S8X2, pitch=w * 2 + 1)       # pitch not a multiple of 2
    shifted_mv = capi.Context.wrap(wide_mv.data + 1, w, h, capi.FORMAT_MV_S8X2, pitch=w * 2 + 2)  # data not 2-byte aligned
    big = ctx.create_frame(w, h)
    mv_in_big = capi.Context.wrap(big.data, w, h, capi.FORMAT_MV_S8X2, pitch=w * 2)  # vectors inside `big`'s bytes
    empty = capi.Frame()
    B = ctypes.byref

    def call(a, b, vi, vo, radius=1):
        return lib.lfg_motion_refine(ctx.h, a and B(a), b and B(b), vi and B(vi), vo and B(vo), radius)

    bad = [
        call(None, c, m, o), call(p, None, m, o), call(p, c, None, o), call(p, c, m, None), call(empty, c, m, o),
        call(p, c, p, o), call(p, m, m, o), call(m, c, m, o), call(p, c, m, p),       # wrong formats
        call(small, c, m, o), call(p, small, m, o), call(p, c, small_mv, o), call(p, c, m, small_mv),  # wrong sizes
        call(odd, c, m, o), call(p, odd, m, o), call(p, c, odd_mv, o), call(p, c, shifted_mv, o), call(p, c, m, odd_mv),
        call(p, c, m, m),                                                              # in place
        call(p, c, mv_in_big, mv_in_big), call(big, c, m, mv_in_big), call(p, big, m, mv_in_big),     # overlaps
        call(p, c, m, o, -1), call(p, c, m, o, 3), call(p, c, m, o, 1000),
    ]
    assert all(rc == -1 for rc in bad), bad                          # LFG_ERR_INVALID
    assert lib.lfg_set_vector_refinement(ctx.h, -2) == -1
    assert lib.lfg_set_vector_refinement(ctx.h, 3) == -1
    assert lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert (ctx.download(o) == pattern).all()
    assert (ctx.download(m) == mv).all()
    # the failed settings changed nothing: lfg_interpolate_frames is still motion + interpolate
    ref = ctx.create_frame(w, h)
    out = ctx.create_frame(w, h)
    ctx.interpolate_frames(p, c, out, 0.5)
    ctx.motion(p, c, m)
    ctx.interpolate(p, c, m, ref, 0.5)
    assert (ctx.download(out) == ctx.download(ref)).all()
    for f in (p, c, m, o, small, small_mv, wide, wide_mv, big, ref, out):
        ctx.destroy_frame(f)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (96, 64), (200, 120), (130, 90), (96, 64), (300, 170)]
    cases = [case(ctx, "random" if i % 2 else "piecewise", w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    alone = [run(ctx, a, b, v, 1 + i % 2) for i, (a, b, v) in enumerate(cases)]

    def enqueue(i, a, b, v):
        h, w = a.shape[:2]
        p, c, m = ctx.frame_from(a), ctx.frame_from(b), ctx.frame_from(v, capi.FORMAT_MV_S8X2)
        o = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
        ctx.motion_refine(p, c, m, o, 1 + i % 2)
        return p, c, m, o

    three_lanes(ctx, cases, enqueue, alone)


# ---- the refinement switch

@pytest.mark.parametrize("estimator", [capi.ESTIMATOR_FULL_SEARCH, capi.ESTIMATOR_PYRAMID])
def test_refinement_switch(ctx, estimator):
    prev, curr, truth, mid, band = rm.moving_objects()
    h, w = prev.shape[:2]
    factors = [0.25, 0.5, 0.75]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    outs = [ctx.create_frame(w, h) for _ in factors]
    ref, rmv = ctx.create_frame(w, h), ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        mv = gpu_vectors(ctx, prev, curr, "full" if estimator == capi.ESTIMATOR_FULL_SEARCH else "pyramid")
        refined = rm.refine(prev, curr, mv, 1)
        ctx.upload(rmv, refined)
        ctx.set_semantics(capi.SEMANTICS_INTENDED)
        ctx.set_motion_estimator(estimator)
        ctx.set_vector_refinement(1)
        # the compensated interpolator: estimator on the GPU, then the refine model, then the compensated model
        ctx.set_interpolator(capi.INTERPOLATOR_COMPENSATED, 48)
        for fused in (False, True):
            ctx.set_fused_motion_interpolate(fused)
            ctx.interpolate_frames(p, c, outs[0], 0.5)
            assert (ctx.download(outs[0]) == mc.interpolate_compensated(prev, curr, refined, 0.5, 48)).all(), fused
            ctx.interpolate_frames_multi(p, c, outs, factors)
            for t, o in zip(factors, outs):
                assert (ctx.download(o) == mc.interpolate_compensated(prev, curr, refined, t, 48)).all(), (fused, t)
        # the shader's interpolation takes the refined vectors too
        ctx.set_interpolator(capi.INTERPOLATOR_SHADER)
        for fused in (False, True):
            ctx.set_fused_motion_interpolate(fused)
            ctx.interpolate_frames(p, c, outs[0], 0.5)
            ctx.interpolate(p, c, rmv, ref, 0.5)
            assert (ctx.download(outs[0]) == ctx.download(ref)).all(), fused
            ctx.interpolate_frames_multi(p, c, outs, factors)
            for t, o in zip(factors, outs):
                ctx.interpolate(p, c, rmv, ref, t)
                assert (ctx.download(o) == ctx.download(ref)).all(), (fused, t)
        ctx.set_fused_motion_interpolate(False)
        # switched back off: the same bytes as a context that never set it
        ctx.set_vector_refinement(-1)
        with capi.Context(0) as fresh:
            fresh.set_semantics(capi.SEMANTICS_INTENDED)
            fresh.set_motion_estimator(estimator)
            fp, fc = fresh.frame_from(prev), fresh.frame_from(curr)
            fo = [fresh.create_frame(w, h) for _ in factors]
            for interp in (capi.INTERPOLATOR_SHADER, capi.INTERPOLATOR_COMPENSATED):
                ctx.set_interpolator(interp)
                fresh.set_interpolator(interp)
                ctx.interpolate_frames(p, c, outs[0], 0.5)
                fresh.interpolate_frames(fp, fc, fo[0], 0.5)
                assert (ctx.download(outs[0]) == fresh.download(fo[0])).all(), interp
                ctx.interpolate_frames_multi(p, c, outs, factors)
                fresh.interpolate_frames_multi(fp, fc, fo, factors)
                for a, b in zip(outs, fo):
                    assert (ctx.download(a) == fresh.download(b)).all(), interp
            for f in [fp, fc] + fo:
                fresh.destroy_frame(f)
    finally:
        ctx.set_vector_refinement(-1)
        ctx.set_interpolator(capi.INTERPOLATOR_SHADER)
        ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
        ctx.set_semantics(capi.SEMANTICS_REFERENCE)
        ctx.set_fused_motion_interpolate(False)
        for f in [p, c, ref, rmv] + outs:
            ctx.destroy_frame(f)


def test_host_refined_stream_matches_capi(tmp_path):
    w, h, n = 1920, 1080, 3
    frames = [synth.make_prev(w, h)]
    for k in range(1, n):
        frames.append(synth.translate(frames[-1], (12, -6), synth.BASE_SEED + k))
    _, got = host_run(tmp_path, frames, (w, h), "--semantics", "intended", "--interpolator", "compensated", "--refine-vectors", "1")
    assert len(got) == 2 * n - 1
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ins = [c.frame_from(f) for f in frames]
        ups = [c.create_frame(w, h) for _ in frames]
        for i, u in zip(ins, ups):
            c.scale(i, u)
        m = c.create_frame(w, h, capi.FORMAT_MV_S8X2)
        r = c.create_frame(w, h, capi.FORMAT_MV_S8X2)
        o = c.create_frame(w, h)
        want = [c.download(ups[0])]
        for k in range(1, n):
            c.motion(ups[k - 1], ups[k], m)
            c.motion_refine(ups[k - 1], ups[k], m, r, 1)
            c.interpolate_compensated(ups[k - 1], ups[k], r, o, 0.5, 48)
            want += [c.download(o), c.download(ups[k])]
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k


# ---- what it is for: the halo around moving edges

def test_moving_square_halo_is_gone(ctx):
    """mc.moving_square with full-search vectors, refined at radius 1.  The refined field is the true one on every pixel
    but the revealed strip (no vector is right there) and three of the square's corners: a corner pixel's 3 x 3 window
    holds 4 texels of the square and 5 of the background.  The generated frames then differ from
    the truth on 6, 6 and 7 pixels, against 36, 33 and 30 without refinement, and with no band left unchecked."""
    prev, curr, (x, y) = mc.moving_square()
    mv = gpu_vectors(ctx, prev, curr, "full")
    h, w = prev.shape[:2]
    truth = np.zeros((h, w, 2), np.int8)
    truth[y:y + 16, x + 12:x + 28] = (-12, 0)
    revealed = np.zeros((h, w), bool)
    revealed[y:y + 16, x:x + 12] = True
    refined = run(ctx, prev, curr, mv, 1)
    assert (refined == rm.refine(prev, curr, mv, 1)).all()
    wrong = np.argwhere((refined != truth).any(-1) & ~revealed)
    assert sorted((int(b) - x - 12, int(a) - y) for a, b in wrong) == [(0, 0), (15, 0), (15, 15)]
    assert int(((mv != truth).any(-1) & ~revealed).sum()) == 27              # the estimator's halo
    bg = np.random.default_rng(7).integers(0, 256, prev.shape, dtype=np.uint8)     # moving_square's own background
    o = ctx.create_frame(w, h)
    p, c, r, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(refined, capi.FORMAT_MV_S8X2), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    try:
        for t, n_refined, n_raw in ((0.25, 6, 36), (0.5, 6, 33), (0.75, 7, 30)):
            s = int(12 * t)
            truth_frame = bg.copy()
            truth_frame[y:y + 16, x + s:x + s + 16] = prev[y:y + 16, x:x + 16]
            ctx.interpolate_compensated(p, c, r, o, t, 48)
            got = ctx.download(o)
            assert (got == mc.interpolate_compensated(prev, curr, refined, t, 48)).all()
            ctx.interpolate_compensated(p, c, m, o, t, 48)
            raw = ctx.download(o)
            assert int((got != truth_frame).any(-1).sum()) == n_refined, t
            assert int((raw != truth_frame).any(-1).sum()) == n_raw, t
    finally:
        for f in (o, p, c, r, m):
            ctx.destroy_frame(f)


def scene_counts(ctx, prev, curr, radius):
    """The pyramid's vectors on the GPU, refined on the GPU, and both compensated frames at t = 0.5."""
    h, w = prev.shape[:2]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    m, r = (ctx.create_frame(w, h, capi.FORMAT_MV_S8X2) for _ in range(2))
    o = ctx.create_frame(w, h)
    try:
        ctx.motion_pyramid(p, c, m, 2, 16, 2)
        ctx.motion_refine(p, c, m, r, radius)
        ctx.interpolate_compensated(p, c, m, o, 0.5, 48)
        raw = ctx.download(o)
        ctx.interpolate_compensated(p, c, r, o, 0.5, 48)
        return ctx.download(m), ctx.download(r), raw, ctx.download(o)
    finally:
        for f in (p, c, m, r, o):
            ctx.destroy_frame(f)


def test_moving_objects_bands(ctx):
    """640 x 360: a synth background panned by (4, -2), a 24 px square moving by (10, 6) and a 40 px one by (-14, 4), the
    pyramid's vectors.  Across the bands within 8 px of every moving edge, the wrong generated pixels at t = 0.5 go from
    220 to 98 (0.45x) with refinement at radius 1, and 75 at radius 2; the wrong vectors on pixels that are not revealed go
    from 1968 to 164 (0.083x).  What remains is the revealed content behind the squares, where no vector is right and the
    choice among wrong ones changes the hole fill."""
    prev, curr, truth, mid, band = rm.moving_objects()
    h, w = prev.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs + truth[..., 0], ys + truth[..., 1]
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    src = np.zeros_like(curr)
    src[ok] = prev[sy[ok], sx[ok]]
    revealed = (src != curr).any(-1)
    for radius, n_after in ((1, 98), (2, 75)):
        mv, refined, raw, got = scene_counts(ctx, prev, curr, radius)
        assert (mv == pm.motion_pyramid(prev, curr, 2, 16, 2)).all()
        assert (refined == rm.refine(prev, curr, mv, radius)).all()
        before = int(((raw != mid).any(-1) & band).sum())
        after = int(((got != mid).any(-1) & band).sum())
        assert (before, after) == (220, n_after), (radius, before, after)
        assert 2 * after < before
        if radius == 1:
            vec_before = int(((mv != truth).any(-1) & band & ~revealed).sum())
            vec_after = int(((refined != truth).any(-1) & band & ~revealed).sum())
            assert (vec_before, vec_after) == (1968, 164)
            assert 4 * vec_after <= vec_before


def test_noise_does_not_pull_interior_pixels(ctx):
    """The same scene with sensor noise of +-4 levels on curr, radius 2: outside the bands refinement does not add wrong
    vectors (7788 before, 4093 after).  More than 16 px from the image's edges it leaves none of the pyramid's 1788; the 64
    pixels it moves off the true vector all lie within 2 px of the edges, where the pan reveals content."""
    prev, curr, truth, mid, band = rm.moving_objects()
    h, w = prev.shape[:2]
    rng = np.random.default_rng(5)
    noisy = np.clip(curr.astype(np.int16) + rng.integers(-4, 5, curr.shape), 0, 255).astype(np.uint8)
    mv, refined, _, _ = scene_counts(ctx, prev, noisy, 2)
    assert (refined == rm.refine(prev, noisy, mv, 2)).all()
    wrong_before, wrong_after = (mv != truth).any(-1) & ~band, (refined != truth).any(-1) & ~band
    assert (int(wrong_before.sum()), int(wrong_after.sum())) == (7788, 4093)
    interior = np.zeros((h, w), bool)
    interior[16:-16, 16:-16] = True
    assert (int((wrong_before & interior).sum()), int((wrong_after & interior).sum())) == (1788, 0)
    pulled = np.argwhere(wrong_after & ~wrong_before)
    assert len(pulled) == 64
    assert all(min(x, w - 1 - x, y, h - 1 - y) <= 2 for y, x in pulled)
