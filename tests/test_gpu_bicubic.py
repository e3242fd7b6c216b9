"""lfg_interpolate_compensated_sampled[_multi] and lfg_set_sampling on the GPU against the CPU model (tests/bicubic_model.py), byte
for byte: both vector formats on the shared cases with padded pitches; the wave-uniform shortcuts both ways; the header's three
anchors; the call equivalences; lanes; argument checks; the switch of lfg_interpolate_frames[_multi] against the route chain's
vectors followed by the model; one 1080p call held on ROIs."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import bicubic_cases as bc
from tests import bicubic_model as bm
from tests import cases
from tests import route_cases as rc
from tests import subpel_cases as sc
from tests import subpel_model as sm
from tests.gpu_kit import ctx, first_bad, three_lanes
from tests.test_gpu_routes import restore, select
from tests.test_gpu_subpel import destroy, pitched

pytestmark = pytest.mark.gpu

MV, MVQ = capi.FORMAT_MV_S8X2, capi.FORMAT_MV_S16X2_Q2
BILINEAR, BICUBIC = capi.SAMPLING_BILINEAR, capi.SAMPLING_BICUBIC
PADS = (3, 5, 7, 9)                                   # pixels of padding on prev, curr, the field and the output


def fmt_of(field):
    return MVQ if field.dtype == np.int16 else MV


class Pitched:
    """A pair and one field on the device, every frame a view with a padded pitch of its own, and one such output."""

    def __init__(self, ctx, prev, curr, field):
        self.ctx, (self.h, self.w) = ctx, prev.shape[:2]
        (self.bp, self.p), (self.bc, self.c) = pitched(ctx, prev, PADS[0]), pitched(ctx, curr, PADS[1])
        self.bm, self.m = pitched(ctx, field, PADS[2], fmt_of(field))
        self.bo, self.o = pitched(ctx, np.zeros((self.h, self.w, 4), np.uint8), PADS[3])

    def run(self, t, match_sad, sampling=BICUBIC):
        self.ctx.interpolate_compensated_sampled(self.p, self.c, self.m, self.o, t, match_sad, sampling)
        raw = self.ctx.download(self.bo)
        assert (raw[:, self.w:] == 0x5A).all(), "bytes beyond the output's rows were written"
        return raw[:, :self.w]

    def close(self):
        destroy(self.ctx, self.bp, self.bc, self.bm, self.bo)


def run_once(ctx, prev, curr, field, t, match_sad, sampling=BICUBIC):
    h, w = prev.shape[:2]
    p, c, m, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(field, fmt_of(field)), ctx.create_frame(w, h)
    try:
        ctx.interpolate_compensated_sampled(p, c, m, o, t, match_sad, sampling)
        return ctx.download(o)
    finally:
        destroy(ctx, p, c, m, o)


# ---- byte for byte against the model

@pytest.mark.parametrize("w,h", bc.SIZES)
def test_both_routes_equal_the_model_on_the_shared_cases(ctx, w, h):
    for name, prev, curr, field in bc.all_cases(sizes=[(w, h)]):
        frames = Pitched(ctx, prev, curr, field)
        try:
            for t in bc.FACTORS + [bc.PHASE_FACTOR]:
                for match_sad in bc.MATCH_SADS:
                    got = frames.run(t, match_sad)
                    want = bm.interpolate(prev, curr, field, t, match_sad)
                    assert (got == want).all(), f"{name} t={t} match_sad={match_sad}: {first_bad(got, want)}"
        finally:
            frames.close()


def test_both_routes_on_a_refined_pan(ctx):
    """Holes at the exposed border, revealed and covered, on real content with real fractions."""
    for wq in sc.PANS[:2]:
        prev, curr, _ = sc.fractional_pan(97, 61, wq)
        mv = sc.pan_vectors(97, 61, wq)
        for field in (sm.refine(prev, curr, mv, 1), mv):
            for t in (0.25, 0.5, 0.7):
                got, want = run_once(ctx, prev, curr, field, t, 48), bm.interpolate(prev, curr, field, t, 48)
                assert (got == want).all(), f"{wq} {field.dtype} t={t}: {first_bad(got, want)}"


# ---- the wave-uniform shortcuts, both ways

@pytest.mark.parametrize("name", sorted(bc.shortcut_fields()))
def test_shortcuts_leave_the_bytes_alone(ctx, name):
    w, h = 130, 9
    field = bc.shortcut_fields(w, h)[name]
    prev, curr = cases.textured(w, h, 5), cases.textured(w, h, 6)
    for match_sad in (1020, 48):
        got, want = run_once(ctx, prev, curr, field, 0.5, match_sad), bm.interpolate(prev, curr, field, 0.5, match_sad)
        assert (got == want).all(), f"{name} match_sad={match_sad}: {first_bad(got, want)}"


# ---- the anchors on the device

def test_anchor_integer_positions_give_the_bilinear_calls_bytes(ctx):
    for name, prev, curr, mv in sc.anchor_inputs():
        h, w = prev.shape[:2]
        p, c = ctx.frame_from(prev), ctx.frame_from(curr)
        m, mq = ctx.frame_from(mv, MV), ctx.frame_from(4 * mv.astype(np.int16), MVQ)
        a, b = ctx.create_frame(w, h), ctx.create_frame(w, h)
        try:
            for t in (0.0, 1.0):
                for match_sad in bc.MATCH_SADS:
                    ctx.interpolate_compensated(p, c, m, a, t, match_sad)
                    want = ctx.download(a)
                    for field in (m, mq):
                        ctx.interpolate_compensated_sampled(p, c, field, b, t, match_sad, BICUBIC)
                        got = ctx.download(b)
                        assert (got == want).all(), (name, t, match_sad, first_bad(got, want))
                    if t == 1.0:
                        assert (want == curr).all()
        finally:
            destroy(ctx, p, c, m, mq, a, b)
    prev, curr = cases.small_scene(130, 21, 5)
    for v in ((2, -4), (-6, 0), (126, -126)):                           # a uniform even vector at t = 0.5
        mv = np.zeros((21, 130, 2), np.int8)
        mv[...] = v
        for match_sad in bc.MATCH_SADS:
            want = run_once(ctx, prev, curr, mv, 0.5, match_sad, BILINEAR)
            assert (run_once(ctx, prev, curr, mv, 0.5, match_sad) == want).all(), (v, match_sad)
            assert (run_once(ctx, prev, curr, 4 * mv.astype(np.int16), 0.5, match_sad) == want).all(), (v, match_sad)


@pytest.mark.parametrize("value", [0, 1, 200, 255])
def test_anchor_constant_frame_stays_constant(ctx, value):
    const = np.full((9, 130, 4), value, np.uint8)
    _, _, mvq, mv = bc.scene("dense", 130, 9, value)
    for field in (mvq, mv):
        for t in (0.3, bc.PHASE_FACTOR):
            assert (run_once(ctx, const, const, field, t, 1020) == value).all()


def test_anchor_step_overshoots_and_clamps(ctx):
    """One pixel per frame at t = 0.5 puts both fetches half a pixel off.  curr is flat, so a pixel is (B + flat) / 2 with B
    the step's fetch: 30, 120, 210 across 40 | 200; across 0 | 255 the clamp holds B to 0 and 255."""
    w, h = 16, 6
    mv = np.zeros((h, w, 2), np.int8)
    mv[...] = (1, 0)
    prev, curr = bm.step(w, h, 40, 200), np.full((h, w, 4), 40, np.uint8)
    got = run_once(ctx, prev, curr, mv, 0.5, 1020)
    assert (got == bm.interpolate(prev, curr, mv, 0.5, 1020)).all()
    assert got[2, 6:9, 0].tolist() == [35, 80, 125]                     # (30 + 40) / 2, (120 + 40) / 2, (210 + 40) / 2
    prev, curr = bm.step(w, h, 0, 255), np.zeros((h, w, 4), np.uint8)
    got = run_once(ctx, prev, curr, mv, 0.5, 1020)
    assert (got == bm.interpolate(prev, curr, mv, 0.5, 1020)).all()
    assert got[2, 6, 0] == 0 and got[2, 7, 0] == 64 and got[2, 8, 0] in (127, 128)   # unclamped: below 0 and 135


# ---- call equivalences

def test_bilinear_is_the_existing_calls(ctx):
    for w, h in ((65, 5), (97, 61)):
        prev, curr, mvq, mv = bc.scene("full_range", w, h, 9)
        p, c, m, q = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, MV), ctx.frame_from(mvq, MVQ)
        a, b = ctx.create_frame(w, h), ctx.create_frame(w, h)
        try:
            for t in bc.FACTORS:
                for match_sad in bc.MATCH_SADS:
                    ctx.interpolate_compensated(p, c, m, a, t, match_sad)
                    ctx.interpolate_compensated_sampled(p, c, m, b, t, match_sad, BILINEAR)
                    assert (ctx.download(a) == ctx.download(b)).all(), (t, match_sad)
                    ctx.interpolate_compensated_subpel(p, c, q, a, t, match_sad)
                    ctx.interpolate_compensated_sampled(p, c, q, b, t, match_sad, BILINEAR)
                    assert (ctx.download(a) == ctx.download(b)).all(), (t, match_sad)
        finally:
            destroy(ctx, p, c, m, q, a, b)


def test_multi_equals_the_single_calls(ctx):
    w, h = 97, 61
    prev, curr, mvq, mv = bc.scene("full_range", w, h, 3)
    factors = bc.FACTORS + [bc.PHASE_FACTOR]
    for field in (mvq, mv):
        p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(field, fmt_of(field))
        outs = [ctx.create_frame(w, h) for _ in factors]
        try:
            ctx.interpolate_compensated_sampled_multi(p, c, m, outs, factors, 48, BICUBIC)
            for t, o in zip(factors, outs):
                got, want = ctx.download(o), bm.interpolate(prev, curr, field, t, 48)
                assert (got == want).all(), (t, first_bad(got, want))
            ctx.interpolate_compensated_sampled(p, c, m, outs[0], factors[2], 48, BICUBIC)       # K reused after the multi call
            assert (ctx.download(outs[0]) == bm.interpolate(prev, curr, field, factors[2], 48)).all()
            ctx.interpolate_compensated_sampled_multi(p, c, m, outs[:2], factors[1:3], 48, BILINEAR)
            assert (ctx.download(outs[1]) == bm.bilinear(prev, curr, field, factors[2], 48)).all()
        finally:
            destroy(ctx, p, c, m, *outs)


def test_hole_reach_does_not_reach_the_bicubic_call(ctx):
    prev, curr, mvq, mv = bc.scene("full_range", 97, 61, 4)
    try:
        ctx.set_hole_reach(32)
        for field in (mvq, mv):
            assert (run_once(ctx, prev, curr, field, 0.5, 48) == bm.interpolate(prev, curr, field, 0.5, 48)).all()
    finally:
        ctx.set_hole_reach(-1)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(130, 70), (97, 61), (130, 70), (65, 33), (97, 61), (160, 90)]
    inputs = []
    for i, (w, h) in enumerate(sizes):
        prev, curr, mvq, mv = bc.scene("full_range", w, h, 60 + i)
        inputs.append((prev, curr, mvq if i % 2 == 0 else mv))
    alone = [bm.interpolate(a, b, v, bc.PHASE_FACTOR, 48) for a, b, v in inputs]

    def enqueue(i, a, b, v):
        h, w = a.shape[:2]
        p, c, m = ctx.frame_from(a), ctx.frame_from(b), ctx.frame_from(v, fmt_of(v))
        o = ctx.create_frame(w, h)
        ctx.interpolate_compensated_sampled(p, c, m, o, bc.PHASE_FACTOR, 48, BICUBIC)
        return p, c, m, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- argument checks

def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 41, 25
    prev, curr, mvq, mv = bc.scene("dense", w, h, 1)
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
    out_in_q = capi.Context.wrap(q.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4)                 # out inside mvq's bytes
    empty = capi.Frame()
    B = ctypes.byref

    def call(a, b, v, o, t=0.5, match_sad=48, sampling=BICUBIC):
        return lib.lfg_interpolate_compensated_sampled(ctx.h, a and B(a), b and B(b), v and B(v), o and B(o), ctypes.c_float(t), match_sad,
                                                       sampling)

    def multi(v, outs, factors, count=None, match_sad=48, sampling=BICUBIC):
        arr = (ctypes.POINTER(capi.Frame) * len(outs))(*[ctypes.pointer(o) for o in outs])
        fs = (ctypes.c_float * len(factors))(*factors)
        return lib.lfg_interpolate_compensated_sampled_multi(ctx.h, B(p), B(c), B(v), arr, fs, len(outs) if count is None else count,
                                                             match_sad, sampling)

    bad = []
    for sampling in (BILINEAR, BICUBIC):
        k = dict(sampling=sampling)
        bad += [
            call(None, c, q, out, **k), call(p, None, q, out, **k), call(p, c, None, out, **k), call(p, c, q, None, **k),
            call(empty, c, q, out, **k), call(p, c, empty, out, **k),
            call(p, c, p, out, **k), call(p, c, q, q, **k), call(q, c, q, out, **k), call(m, c, m, out, **k), call(p, c, m, m, **k),   # formats
            call(small, c, q, out, **k), call(p, c, small_q, out, **k), call(p, c, small_mv, out, **k), call(p, c, q, small, **k),  # sizes
            call(odd, c, q, out, **k), call(p, shifted, m, out, **k), call(p, c, odd_q, out, **k), call(p, c, shifted_q, out, **k),
            call(p, c, odd_mv, out, **k), call(p, c, shifted_mv, out, **k), call(p, c, q, odd, **k),                                # alignment
            call(p, c, q, p, **k), call(p, c, m, c, **k), call(p, c, q, out_in_q, **k),                                             # overlaps
            call(p, c, q, out, -0.01, **k), call(p, c, m, out, 1.01, **k), call(p, c, q, out, float("nan"), **k),
            call(p, c, m, out, float("inf"), **k), call(p, c, q, out, 0.5, -1, **k), call(p, c, m, out, 0.5, 1021, **k),
            multi(q, [out, out2], [0.5, 0.25], 0, **k), multi(m, [out, out2] * 9, [0.5] * 18, **k), multi(q, [out, out], [0.5, 0.25], **k),
            multi(m, [out, out2], [0.5, 2.0], **k), multi(q, [out, out2], [0.5, 0.25], None, 2000, **k),
        ]
    for sampling in (-1, 2, 100):                                      # an unknown sampling, with everything else in order
        bad += [call(p, c, q, out, sampling=sampling), call(p, c, m, out, sampling=sampling), multi(q, [out, out2], [0.5, 0.25], sampling=sampling)]
    assert all(code == -1 for code in bad), bad                        # LFG_ERR_INVALID
    assert "sampling" in lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_interpolate_compensated_sampled(None, B(p), B(c), B(q), B(out), ctypes.c_float(0.5), 48, BICUBIC) == -1
    for value in (-1, 2, 100):
        assert lib.lfg_set_sampling(ctx.h, value) == -1
    assert "lfg_set_sampling" in lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_set_sampling(None, BICUBIC) == -1 and lib.lfg_sampling_effective(None) == BILINEAR
    assert ctx.sampling_effective() == BILINEAR
    ctx.sync()
    assert (ctx.download(out) == out_pattern).all()
    assert (ctx.download(q) == mvq).all() and (ctx.download(m) == mv).all() and (ctx.download(p) == prev).all()
    destroy(ctx, p, c, m, q, out, out2, small, small_q, small_mv, wide, wide_q, wide_mv)


# ---- the switch of lfg_interpolate_frames[_multi]

FACTORS = [0.25, 0.5, bc.PHASE_FACTOR]
ROUTES = [rc.route(("pyramid", 1, "compensated", 1)), rc.route(("pyramid", 1, "compensated", 1), subpel=1),
          rc.route(("full", 0, "compensated", 1)), rc.route(("full", 0, "compensated", 1), subpel=1)]


@pytest.fixture(scope="module")
def scene(ctx):
    chain = rc.scene_chain()
    h, w = chain.prev.shape[:2]
    p, c = ctx.frame_from(chain.prev), ctx.frame_from(chain.curr)
    outs = [ctx.create_frame(w, h) for _ in FACTORS]
    yield chain, p, c, outs
    destroy(ctx, p, c, *outs)


def field_of(chain, r):
    """The field the route's sampling kernel reads: the chain's final integer vectors, to quarter pixels where they apply."""
    fwd, _ = chain.vectors(r)
    return sm.refine(chain.prev, chain.curr, fwd, r.subpel) if r.subpel >= 0 else fwd


def off(ctx):
    ctx.set_sampling(BILINEAR)
    restore(ctx)


@pytest.mark.parametrize("r", ROUTES, ids=rc.route_id)
def test_switch_equals_the_chains_vectors_and_the_model(ctx, scene, r):
    chain, p, c, outs = scene
    field = field_of(chain, r)
    try:
        select(ctx, chain, r)
        ctx.set_sampling(BICUBIC)
        assert ctx.sampling_effective() == BICUBIC
        ctx.interpolate_frames(p, c, outs[0], FACTORS[0])
        got = ctx.download(outs[0])
        want = bm.interpolate(chain.prev, chain.curr, field, FACTORS[0], r.match_sad)
        assert (got == want).all(), first_bad(got, want)
        ctx.interpolate_frames_multi(p, c, outs, FACTORS)
        for t, o in zip(FACTORS, outs):
            got, want = ctx.download(o), bm.interpolate(chain.prev, chain.curr, field, t, r.match_sad)
            assert (got == want).all(), (t, first_bad(got, want))
        assert (want != chain.frames(r, [FACTORS[-1]])[0]).any()              # the fetch changes the frame
        ctx.set_sampling(BILINEAR)                                           # and off again: the route's own frame
        ctx.interpolate_frames(p, c, outs[0], FACTORS[1])
        assert (ctx.download(outs[0]) == chain.frames(r, [FACTORS[1]])[0]).all()
    finally:
        off(ctx)


LAPSES = [dict(interpolator="shader"), dict(generation="extrapolate"), dict(protect=8), dict(bidirectional=1), dict(reach=32), dict(reach=16),
          dict(protect=0, bidirectional=1, subpel=1), dict(reach=255, subpel=1)]


@pytest.mark.parametrize("change", LAPSES, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_settings_under_which_the_switch_lapses(ctx, scene, change):
    chain, p, c, outs = scene
    r = rc.route(("pyramid", 1, "compensated", 1))._replace(**change)
    try:
        select(ctx, chain, r)
        ctx.set_sampling(BICUBIC)
        assert ctx.sampling_effective() == BILINEAR
        ctx.interpolate_frames_multi(p, c, outs[:2], FACTORS[:2])
        for o, want in zip(outs, chain.frames(r, FACTORS[:2])):
            got = ctx.download(o)
            assert (got == want).all(), first_bad(got, want)
    finally:
        off(ctx)


def test_switch_changed_between_enqueued_calls(ctx, scene):
    """Nothing waits between the calls: each takes the setting of the moment it was enqueued."""
    chain, p, c, outs = scene
    r = ROUTES[1]
    field = field_of(chain, r)
    try:
        select(ctx, chain, r)
        for o, sampling in zip(outs, (BICUBIC, BILINEAR, BICUBIC)):
            ctx.set_sampling(sampling)
            ctx.interpolate_frames(p, c, o, 0.5)
        want = {BICUBIC: bm.interpolate(chain.prev, chain.curr, field, 0.5, r.match_sad), BILINEAR: chain.frames(r, [0.5])[0]}
        for o, sampling in zip(outs, (BICUBIC, BILINEAR, BICUBIC)):
            assert (ctx.download(o) == want[sampling]).all(), sampling
    finally:
        off(ctx)


def test_a_change_of_size(ctx):
    r = ROUTES[1]
    try:
        for i, (w, h) in enumerate([(96, 64), (33, 17), (1, 1), (97, 64), (96, 64)]):
            prev, curr, _ = sc.fractional_pan(w, h, (10, -6), seed=40 + i)
            chain = rc.RouteChain(prev, curr)
            p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
            try:
                select(ctx, chain, r)
                ctx.set_sampling(BICUBIC)
                ctx.interpolate_frames(p, c, o, 0.5)
                got, want = ctx.download(o), bm.interpolate(prev, curr, field_of(chain, r), 0.5, r.match_sad)
                assert (got == want).all(), (w, h, first_bad(got, want))
            finally:
                destroy(ctx, p, c, o)
    finally:
        off(ctx)


# ---- one large call

def test_1080p_on_eight_rois(ctx):
    w, h = 1920, 1080
    prev, curr, mvq, _ = bc.scene("dense", w, h, 77)
    mvq[:, :960] = (8, -16)                                            # whole waves on the single-texel path too
    t = 0.5
    got = run_once(ctx, prev, curr, mvq, t, 48)
    K = bm.keys(prev, curr, mvq, t, 48)
    for x, y in ((0, 0), (w - 64, 0), (0, h - 64), (w - 64, h - 64), (928, 500), (448, 300), (1400, 700), (960, 1016)):
        want = bm.sample(prev, curr, mvq, K, t, 48, roi=(x, y, 64, 64))
        assert (got[y:y + 64, x:x + 64] == want).all(), ((x, y), first_bad(got[y:y + 64, x:x + 64], want))
