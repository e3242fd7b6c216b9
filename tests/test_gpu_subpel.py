"""lfg_motion_subpel and lfg_interpolate_compensated_subpel[_multi] on the GPU against the CPU model (tests/subpel_model.py),
byte for byte; the anchor against lfg_interpolate_compensated; pitches; lanes; argument checks; the switch of
lfg_interpolate_frames[_multi] (lfg_set_subpixel_vectors) against the chain of public calls; the host's --subpel-vectors."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import cases
from tests import subpel_cases as sc
from tests import subpel_model as sm
from tests.gpu_kit import ESTIMATOR, ctx, first_bad, host_run, three_lanes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (65, 5), (97, 61), (130, 9)]        # below, across and past the 64 x 4 block on both axes
RADII = [0, 1, 2]
MV, MVQ = capi.FORMAT_MV_S8X2, capi.FORMAT_MV_S16X2_Q2


def destroy(ctx, *frames):
    for f in frames:
        ctx.destroy_frame(f)


def pitched(ctx, host, pad_px, fmt=capi.FORMAT_RGBA8):
    """`host` in the left part of a wider frame, described with the wider row pitch; the padding poisoned with 0x5A bytes.
    Returns (the wider frame, the view)."""
    h, w, ch = host.shape
    wide = np.full((h, w + pad_px, ch), 0x5A5A if host.dtype == np.int16 else 0x5A, host.dtype)
    wide[:, :w] = host
    big = ctx.frame_from(wide, fmt)
    return big, capi.Context.wrap(big.data, w, h, fmt, pitch=(w + pad_px) * ch * host.itemsize)


def run_subpel(ctx, prev, curr, mv, radius, pads=None):
    """lfg_motion_subpel; with pads = (prev, curr, mv, out) pixels of padding every frame is a view with a pitch of its own."""
    h, w = prev.shape[:2]
    if pads is None:
        p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, MV)
        o = ctx.create_frame(w, h, MVQ)
        try:
            ctx.motion_subpel(p, c, m, o, radius)
            return ctx.download(o)
        finally:
            destroy(ctx, p, c, m, o)
    (bp, p), (bc, c), (bm, m) = pitched(ctx, prev, pads[0]), pitched(ctx, curr, pads[1]), pitched(ctx, mv, pads[2], MV)
    bo, o = pitched(ctx, np.zeros((h, w, 2), np.int16), pads[3], MVQ)
    try:
        ctx.motion_subpel(p, c, m, o, radius)
        raw = ctx.download(bo)
        assert (raw[:, w:] == 0x5A5A).all()
        return raw[:, :w]
    finally:
        destroy(ctx, bp, bc, bm, bo)


def run_route(ctx, prev, curr, mvq, t, match_sad, pads=None):
    h, w = prev.shape[:2]
    if pads is None:
        p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mvq, MVQ)
        o = ctx.create_frame(w, h)
        try:
            ctx.interpolate_compensated_subpel(p, c, m, o, t, match_sad)
            return ctx.download(o)
        finally:
            destroy(ctx, p, c, m, o)
    (bp, p), (bc, c), (bm, m) = pitched(ctx, prev, pads[0]), pitched(ctx, curr, pads[1]), pitched(ctx, mvq, pads[2], MVQ)
    bo, o = pitched(ctx, np.zeros((h, w, 4), np.uint8), pads[3])
    try:
        ctx.interpolate_compensated_subpel(p, c, m, o, t, match_sad)
        raw = ctx.download(bo)
        assert (raw[:, w:] == 0x5A).all()
        return raw[:, :w]
    finally:
        destroy(ctx, bp, bc, bm, bo)


def pads_of(w, h):
    return (3, 5, 7, 9) if (w, h) == (130, 9) else None      # 130 x 9: padded pitches on every frame


# ---- lfg_motion_subpel

@pytest.mark.parametrize("w,h", SIZES)
def test_subpel_equals_the_model_on_pans_and_random_vectors(ctx, w, h):
    inputs = [(f"pan{wq}", *sc.fractional_pan(w, h, wq)[:2], sc.pan_vectors(w, h, wq)) for wq in sc.PANS]
    inputs.append(("random", *sc.random_vectors(w, h, 31 * w + h)))
    for name, prev, curr, mv in inputs:
        for radius in RADII:
            got = run_subpel(ctx, prev, curr, mv, radius, pads_of(w, h))
            want = sm.refine(prev, curr, mv, radius)
            assert (got == want).all(), f"{w}x{h} {name} radius={radius}: {first_bad(got, want)}"
            assert np.abs(got.astype(int)).max() <= sm.LIMIT


@pytest.mark.parametrize("name", sorted(sc.KNOWN))
def test_subpel_known_answers(ctx, name):
    prev, curr, mv, radius, want = sc.KNOWN[name]()
    got = run_subpel(ctx, prev, curr, mv, radius)
    bad = [(q, tuple(int(c) for c in got[q[1], q[0]]), v) for q, v in want.items() if tuple(got[q[1], q[0]]) != v]
    assert not bad, bad[:4]
    for r in RADII:
        got, model = run_subpel(ctx, prev, curr, mv, r), sm.refine(prev, curr, mv, r)
        assert (got == model).all(), f"{name} radius={r}: {first_bad(got, model)}"


def test_subpel_recovers_a_fractional_pan(ctx):
    wq = (10, -6)
    prev, curr, _ = sc.fractional_pan(96, 64, wq)
    got = run_subpel(ctx, prev, curr, sc.pan_vectors(96, 64, wq), 1)
    assert (sc.interior(got) == np.array(wq)).all()


# ---- lfg_interpolate_compensated_subpel

@pytest.mark.parametrize("w,h", SIZES)
def test_route_equals_the_model_on_random_vectors(ctx, w, h):
    prev, curr, mvq = sc.random_mvq(w, h, 17 * w + h)
    for t in sc.FACTORS:
        for match_sad in sc.MATCH_SADS:
            got = run_route(ctx, prev, curr, mvq, t, match_sad, pads_of(w, h))
            want = sm.interpolate(prev, curr, mvq, t, match_sad)
            assert (got == want).all(), f"{w}x{h} t={t} match_sad={match_sad}: {first_bad(got, want)}"
    assert (run_route(ctx, prev, curr, mvq, 1.0, 48) == curr).all()


def test_route_equals_the_model_on_a_refined_pan(ctx):
    """Holes at the exposed border, revealed and covered, with real fractions: the pan's refined field."""
    for wq in sc.PANS[:2]:
        prev, curr, _ = sc.fractional_pan(97, 61, wq)
        mvq = sm.refine(prev, curr, sc.pan_vectors(97, 61, wq), 1)
        for t in (0.25, 0.5, 0.7):
            got, want = run_route(ctx, prev, curr, mvq, t, 48), sm.interpolate(prev, curr, mvq, t, 48)
            assert (got == want).all(), f"{wq} t={t}: {first_bad(got, want)}"


def test_route_collision_and_holes(ctx):
    prev, curr, mvq, (x, y), winner = sc.collision()
    got = run_route(ctx, prev, curr, mvq, sc.COLLISION_FACTOR, 0)
    assert (got == sm.interpolate(prev, curr, mvq, sc.COLLISION_FACTOR, 0)).all()
    # textured frames at match_sad 1020, where every pixel matches too and the bytes show which vector a pixel was sampled with
    prev, curr = cases.textured(8, 8, 61), cases.textured(8, 8, 62)
    got, want = run_route(ctx, prev, curr, mvq, sc.COLLISION_FACTOR, 1020), sm.interpolate(prev, curr, mvq, sc.COLLISION_FACTOR, 1020)
    assert (got == want).all(), first_bad(got, want)
    K = sm.keys(prev, curr, mvq, sc.COLLISION_FACTOR, 1020)
    assert int(K[y, x]) == sm.key(*winner)
    loser = K.copy()
    loser[y, x] = np.uint64(sm.key(-9, 0))
    assert (sm.sample(prev, curr, mvq, loser, sc.COLLISION_FACTOR, 1020)[y, x] != got[y, x]).any()      # the other order shows
    prev, curr, mvq, obj = sc.revealed_and_covered()
    got = run_route(ctx, prev, curr, mvq, 0.5, 0)
    assert (got == sm.interpolate(prev, curr, mvq, 0.5, 0)).all()
    assert (got[2, 5] == obj).all() and (got[2, 4] == curr[2, 4]).all() and (got[2, 6] == prev[2, 6]).all()


def test_multi_equals_the_single_calls(ctx):
    w, h = 97, 61
    prev, curr, mvq = sc.random_mvq(w, h, 3)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mvq, MVQ)
    outs = [ctx.create_frame(w, h) for _ in sc.FACTORS]
    try:
        ctx.interpolate_compensated_subpel_multi(p, c, m, outs, sc.FACTORS, 48)
        for t, o in zip(sc.FACTORS, outs):
            got, want = ctx.download(o), sm.interpolate(prev, curr, mvq, t, 48)
            assert (got == want).all(), (t, first_bad(got, want))
        ctx.interpolate_compensated_subpel(p, c, m, outs[0], sc.FACTORS[2], 48)      # K reused after the multi call
        assert (ctx.download(outs[0]) == sm.interpolate(prev, curr, mvq, sc.FACTORS[2], 48)).all()
    finally:
        destroy(ctx, p, c, m, *outs)


def test_anchor_on_the_device(ctx):
    """lfg_interpolate_compensated_subpel(4 mv) equals lfg_interpolate_compensated(mv), byte for byte."""
    for name, prev, curr, mv in sc.anchor_inputs():
        h, w = prev.shape[:2]
        p, c = ctx.frame_from(prev), ctx.frame_from(curr)
        m, mq = ctx.frame_from(mv, MV), ctx.frame_from(4 * mv.astype(np.int16), MVQ)
        a, b = ctx.create_frame(w, h), ctx.create_frame(w, h)
        try:
            for t in sc.FACTORS:
                for match_sad in sc.MATCH_SADS:
                    ctx.interpolate_compensated(p, c, m, a, t, match_sad)
                    ctx.interpolate_compensated_subpel(p, c, mq, b, t, match_sad)
                    want, got = ctx.download(a), ctx.download(b)
                    assert (got == want).all(), (name, t, match_sad, first_bad(got, want))
        finally:
            destroy(ctx, p, c, m, mq, a, b)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(130, 70), (97, 61), (130, 70), (65, 33), (97, 61), (160, 90)]
    inputs = [sc.random_mvq(w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    alone = [run_route(ctx, a, b, v, 0.5, 48) for a, b, v in inputs]

    def enqueue(i, a, b, v):
        h, w = a.shape[:2]
        p, c, m = ctx.frame_from(a), ctx.frame_from(b), ctx.frame_from(v, MVQ)
        o = ctx.create_frame(w, h)
        ctx.interpolate_compensated_subpel(p, c, m, o, 0.5, 48)
        return p, c, m, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- argument checks

def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 41, 25
    prev, curr, mv = sc.random_vectors(w, h, 1)
    mvq = sm.refine(prev, curr, mv, 1)
    p, c, m, q = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, MV), ctx.frame_from(mvq, MVQ)
    out = ctx.create_frame(w, h)
    out_pattern = np.full((h, w, 4), 0x5A, np.uint8)
    ctx.upload(out, out_pattern)
    out2 = ctx.create_frame(w, h)
    small, small_q, small_mv = ctx.create_frame(w - 1, h), ctx.create_frame(w, h - 1, MVQ), ctx.create_frame(w - 1, h, MV)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)              # pitch not a multiple of 4
    shifted = capi.Context.wrap(wide.data + 2, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 4)      # data not 4-byte aligned
    wide_q = ctx.create_frame(w + 1, h, MVQ)
    odd_q = capi.Context.wrap(wide_q.data, w, h, MVQ, pitch=w * 4 + 2)
    shifted_q = capi.Context.wrap(wide_q.data + 2, w, h, MVQ, pitch=w * 4 + 4)
    wide_mv = ctx.create_frame(w + 1, h, MV)
    odd_mv = capi.Context.wrap(wide_mv.data, w, h, MV, pitch=w * 2 + 1)
    shifted_mv = capi.Context.wrap(wide_mv.data + 1, w, h, MV, pitch=w * 2 + 2)
    q_in_p = capi.Context.wrap(p.data, w, h, MVQ, pitch=w * 4)                                 # mvq_out inside prev's bytes
    mv_in_q = capi.Context.wrap(q.data, w, h, MV, pitch=w * 4)                                 # mv_in inside mvq_out's bytes
    out_in_q = capi.Context.wrap(q.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4)                 # out inside mvq's bytes
    empty = capi.Frame()
    B = ctypes.byref

    def subpel(a, b, vi, vo, radius=1):
        return lib.lfg_motion_subpel(ctx.h, a and B(a), b and B(b), vi and B(vi), vo and B(vo), radius)

    def route(a, b, v, o, t=0.5, match_sad=48):
        return lib.lfg_interpolate_compensated_subpel(ctx.h, a and B(a), b and B(b), v and B(v), o and B(o), ctypes.c_float(t), match_sad)

    def multi(outs, factors, count=None, match_sad=48):
        arr = (ctypes.POINTER(capi.Frame) * len(outs))(*[ctypes.pointer(o) for o in outs])
        fs = (ctypes.c_float * len(factors))(*factors)
        return lib.lfg_interpolate_compensated_subpel_multi(ctx.h, B(p), B(c), B(q), arr, fs, len(outs) if count is None else count, match_sad)

    bad = [
        subpel(None, c, m, q), subpel(p, None, m, q), subpel(p, c, None, q), subpel(p, c, m, None), subpel(empty, c, m, q),
        subpel(p, c, q, q), subpel(p, c, m, m), subpel(p, c, m, out), subpel(m, c, m, q), subpel(p, q, m, q),       # wrong formats
        subpel(small, c, m, q), subpel(p, small, m, q), subpel(p, c, small_mv, q), subpel(p, c, m, small_q),        # wrong sizes
        subpel(odd, c, m, q), subpel(p, odd, m, q), subpel(shifted, c, m, q), subpel(p, c, odd_mv, q), subpel(p, c, shifted_mv, q),
        subpel(p, c, m, odd_q), subpel(p, c, m, shifted_q),                                                         # alignment
        subpel(p, c, m, q_in_p), subpel(p, c, mv_in_q, q),                                                          # overlaps
        subpel(p, c, m, q, -1), subpel(p, c, m, q, 3), subpel(p, c, m, q, 1000),                                    # radius
        route(None, c, q, out), route(p, None, q, out), route(p, c, None, out), route(p, c, q, None), route(empty, c, q, out),
        route(p, c, m, out), route(p, c, q, q), route(q, c, q, out),                                                # wrong formats
        route(small, c, q, out), route(p, c, small_q, out), route(p, c, q, small),                                  # wrong sizes
        route(odd, c, q, out), route(p, shifted, q, out), route(p, c, odd_q, out), route(p, c, shifted_q, out), route(p, c, q, odd),
        route(p, c, q, p), route(p, c, q, c), route(p, c, q, out_in_q),                                             # overlaps
        route(p, c, q, out, -0.01), route(p, c, q, out, 1.01), route(p, c, q, out, float("nan")), route(p, c, q, out, float("inf")),
        route(p, c, q, out, 0.5, -1), route(p, c, q, out, 0.5, 1021),
        multi([out, out2], [0.5, 0.25], 0), multi([out, out2] * 9, [0.5] * 18), multi([out, out], [0.5, 0.25]),
        multi([out, out2], [0.5, 2.0]), multi([out, out2], [0.5, 0.25], None, 2000),
    ]
    assert all(rc == -1 for rc in bad), bad                          # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    for value in (-2, 3, 100):
        assert lib.lfg_set_subpixel_vectors(ctx.h, value) == -1
    assert "lfg_set_subpixel_vectors" in lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert (ctx.download(out) == out_pattern).all()
    assert (ctx.download(q) == mvq).all() and (ctx.download(m) == mv).all() and (ctx.download(p) == prev).all()
    destroy(ctx, p, c, m, q, out, out2, small, small_q, small_mv, wide, wide_q, wide_mv)


def test_frames_of_the_format_copy_upload_and_download(ctx):
    w, h = 33, 7
    mvq = np.random.default_rng(2).integers(-32768, 32768, (h, w, 2)).astype(np.int16)
    a, b = ctx.frame_from(mvq, MVQ), ctx.create_frame(w, h, MVQ)
    try:
        assert a.pitch == w * 4 and a.format == MVQ
        ctx.copy(a, b)
        assert (ctx.download(b) == mvq).all()
        with pytest.raises(capi.LfgError):
            capi.Context.wrap(a.data, w, h, MVQ, pitch=w * 4 - 1)     # pitch below a row
    finally:
        destroy(ctx, a, b)


# ---- the switch of lfg_interpolate_frames[_multi]

FACTORS = [0.25, 0.5, 0.9]
PAN = (10, -6)


class Pair:
    """A pair on the device, with every frame the chain of public calls needs."""

    def __init__(self, ctx, prev, curr):
        self.ctx, (self.h, self.w) = ctx, prev.shape[:2]
        w, h = self.w, self.h
        self.p, self.c = ctx.frame_from(prev), ctx.frame_from(curr)
        self.mv, self.refined, self.mvq = ctx.create_frame(w, h, MV), ctx.create_frame(w, h, MV), ctx.create_frame(w, h, MVQ)
        self.outs = [ctx.create_frame(w, h) for _ in FACTORS]
        self.ref = ctx.create_frame(w, h)

    def close(self):
        destroy(self.ctx, self.p, self.c, self.mv, self.refined, self.mvq, self.ref, *self.outs)

    def chain(self, estimator, refine, radius, factors):
        """The public calls that the switch stands for: the generated frames, downloaded."""
        ctx = self.ctx
        if estimator == "full":
            ctx.motion(self.p, self.c, self.mv)
        else:
            ctx.motion_pyramid(self.p, self.c, self.mv, 2, 16, 2)
        field = self.mv
        if refine >= 0:
            ctx.motion_refine(self.p, self.c, self.mv, self.refined, refine)
            field = self.refined
        ctx.motion_subpel(self.p, self.c, field, self.mvq, radius)
        out = []
        for t in factors:
            ctx.interpolate_compensated_subpel(self.p, self.c, self.mvq, self.ref, t, 48)
            out.append(ctx.download(self.ref))
        return out


def select(ctx, estimator="pyramid", refine=-1, radius=-1, interpolator=capi.INTERPOLATOR_COMPENSATED):
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    ctx.set_motion_estimator(ESTIMATOR[estimator])
    ctx.set_vector_refinement(refine)
    ctx.set_interpolator(interpolator, 48)
    ctx.set_subpixel_vectors(radius)


def deselect(ctx):
    select(ctx, "full", -1, -1, capi.INTERPOLATOR_SHADER)
    ctx.set_semantics(capi.SEMANTICS_REFERENCE)
    ctx.set_generation(capi.GENERATION_INTERPOLATE)
    ctx.set_bidirectional(-1)
    ctx.set_static_protection(-1)
    ctx.set_hole_reach(-1)
    ctx.set_cut_detection(-1)
    ctx.set_fused_motion_interpolate(False)


@pytest.fixture(scope="module")
def pan_pair(ctx):
    prev, curr, _ = sc.fractional_pan(200, 120, PAN)
    pair = Pair(ctx, prev, curr)
    yield pair
    pair.close()


@pytest.mark.parametrize("estimator,refine,radius", [("full", -1, 1), ("pyramid", -1, 0), ("pyramid", 1, 1), ("full", 0, 2)])
def test_switch_equals_the_chain_of_public_calls(ctx, pan_pair, estimator, refine, radius):
    pair = pan_pair
    try:
        select(ctx, estimator, refine, radius)
        want = pair.chain(estimator, refine, radius, FACTORS)
        for fused in (False, True):
            ctx.set_fused_motion_interpolate(fused)
            ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], FACTORS[0])
            got = ctx.download(pair.outs[0])
            assert (got == want[0]).all(), (fused, first_bad(got, want[0]))
        ctx.set_fused_motion_interpolate(False)
        ctx.interpolate_frames_multi(pair.p, pair.c, pair.outs, FACTORS)
        for t, o, e in zip(FACTORS, pair.outs, want):
            got = ctx.download(o)
            assert (got == e).all(), (t, first_bad(got, e))
        ctx.set_cut_detection(0)                                       # detection on, never a cut: the same frames
        ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], FACTORS[1])
        assert (ctx.download(pair.outs[0]) == want[1]).all()
    finally:
        deselect(ctx)


def test_off_and_every_setting_that_switches_the_route_off(ctx, pan_pair):
    pair = pan_pair

    def frame():
        ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], 0.5)
        return ctx.download(pair.outs[0])

    try:
        select(ctx)
        before = frame()
        ctx.set_subpixel_vectors(1)
        on = frame()
        assert (on == pair.chain("pyramid", -1, 1, [0.5])[0]).all()
        assert (on != before).any()                                      # the route changes the frame on a fractional pan
        assert ctx.lib.lfg_set_subpixel_vectors(ctx.h, 3) == -1          # refused: still radius 1
        assert (frame() == on).all()
        ctx.set_subpixel_vectors(-1)
        assert (frame() == before).all()
        # with -1 the frame is today's: the integer chain of public calls
        ctx.motion_pyramid(pair.p, pair.c, pair.mv, 2, 16, 2)
        ctx.interpolate_compensated(pair.p, pair.c, pair.mv, pair.ref, 0.5, 48)
        assert (ctx.download(pair.ref) == before).all()
        offs = {
            "shader": lambda on_: ctx.set_interpolator(capi.INTERPOLATOR_SHADER if on_ else capi.INTERPOLATOR_COMPENSATED, 48),
            "extrapolate": lambda on_: ctx.set_generation(capi.GENERATION_EXTRAPOLATE if on_ else capi.GENERATION_INTERPOLATE),
            "bidirectional": lambda on_: ctx.set_bidirectional(2 if on_ else -1),
            "static": lambda on_: ctx.set_static_protection(8 if on_ else -1),
            "hole_reach": lambda on_: ctx.set_hole_reach(32 if on_ else -1),
        }
        for name, setting in offs.items():
            setting(True)
            try:
                ctx.set_subpixel_vectors(-1)
                without = frame()
                ctx.set_subpixel_vectors(1)
                assert (frame() == without).all(), name
            finally:
                setting(False)
        assert (frame() == on).all()                                     # and on again once they are off
    finally:
        deselect(ctx)


def test_temporaries_follow_a_change_of_size(ctx):
    try:
        for i, (w, h) in enumerate([(96, 64), (33, 17), (1, 1), (97, 64), (96, 64)]):
            prev, curr, _ = sc.fractional_pan(w, h, PAN, seed=40 + i)
            pair = Pair(ctx, prev, curr)
            try:
                select(ctx, "pyramid", -1, 1)
                want = pair.chain("pyramid", -1, 1, [0.5])[0]
                ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], 0.5)
                got = ctx.download(pair.outs[0])
                assert (got == want).all(), (w, h, first_bad(got, want))
            finally:
                pair.close()
    finally:
        deselect(ctx)


def test_lanes_in_flight_share_neither_k_nor_the_temporary(ctx):
    sizes = [(130, 70), (97, 61), (130, 70), (65, 33), (97, 61), (160, 90)]
    inputs = [sc.fractional_pan(w, h, sc.PANS[i % 4], seed=80 + i)[:2] for i, (w, h) in enumerate(sizes)]
    try:
        select(ctx, "pyramid", -1, 1)

        def one(a, b):
            h, w = a.shape[:2]
            p, c, o = ctx.frame_from(a), ctx.frame_from(b), ctx.create_frame(w, h)
            try:
                ctx.interpolate_frames(p, c, o, 0.5)
                return ctx.download(o)
            finally:
                destroy(ctx, p, c, o)

        alone = [one(a, b) for a, b in inputs]

        def enqueue(i, a, b):
            h, w = a.shape[:2]
            p, c, o = ctx.frame_from(a), ctx.frame_from(b), ctx.create_frame(w, h)
            ctx.interpolate_frames(p, c, o, 0.5)
            return p, c, o

        three_lanes(ctx, inputs, enqueue, alone)
    finally:
        deselect(ctx)


# ---- the host

@pytest.mark.parametrize("in_flight", [1, 3])
def test_host_stream_equals_the_chain(tmp_path, in_flight):
    w, h, n = 160, 96, 8
    frames = sc.pan_stream(w, h, PAN, n)
    info, got = host_run(tmp_path, frames, (w, h), "--motion", "pyramid", "--interpolator", "compensated", "--semantics", "intended",
                         "--subpel-vectors", "1", "--in-flight", in_flight)
    assert info["subpel_vectors"] == 1
    assert len(got) == 2 * n - 1
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ins = [c.frame_from(f) for f in frames]
        ups = [c.create_frame(w, h) for _ in frames]
        for i, u in zip(ins, ups):
            c.scale(i, u)
        m, q, o = c.create_frame(w, h, MV), c.create_frame(w, h, MVQ), c.create_frame(w, h)
        want = [c.download(ups[0])]
        for k in range(1, n):
            c.motion_pyramid(ups[k - 1], ups[k], m, 2, 16, 2)
            c.motion_subpel(ups[k - 1], ups[k], m, q, 1)
            c.interpolate_compensated_subpel(ups[k - 1], ups[k], q, o, 0.5, 48)
            want += [c.download(o), c.download(ups[k])]
        c.motion_pyramid(ups[0], ups[1], m, 2, 16, 2)
        c.interpolate_compensated(ups[0], ups[1], m, o, 0.5, 48)
        plain = c.download(o)
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k
    assert (got[1] != plain).any()                                       # the flag changes the stream
