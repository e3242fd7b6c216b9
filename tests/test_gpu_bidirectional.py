"""lfg_interpolate_compensated_bidirectional and lfg_motion_consistency on the GPU against the CPU model
(tests/bidir_model.py), byte for byte; lfg_set_bidirectional behind lfg_interpolate_frames[_multi] against the explicit sequence
of calls; argument checks; lanes; lfg_host --bidirectional."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import bidir_cases as bc
from tests import bidir_model as bd
from tests import cases
from tests.gpu_kit import DEFAULT, apply, ctx, first_bad, gpu_vectors, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

# one pixel, ragged, not a multiple of the 64 x 4 workgroup, exactly one workgroup column, several with a remainder
SIZES = [(1, 1), (7, 5), (33, 17), (64, 64), (257, 131)]
KINDS = list(bc.FIELDS) + ["motion", "pyramid"]
COMPENSATED = ("full", -1, "compensated", capi.SEMANTICS_INTENDED)
MV = capi.FORMAT_MV_S8X2


def case(ctx, kind, w, h, seed):
    """(prev, curr, fwd, bwd) for one kind of field pair: an estimator run both ways on the GPU, or one of bidir_cases.field."""
    if kind in ("motion", "pyramid"):
        prev, curr = cases.small_scene(w, h, seed)
        if kind == "pyramid" and min(w, h) >= 64:
            curr = synth.translate(prev, (-30, 18), synth.BASE_SEED + seed)
        estimator = "full" if kind == "motion" else "pyramid"
        return prev, curr, gpu_vectors(ctx, prev, curr, estimator), gpu_vectors(ctx, curr, prev, estimator)
    return bc.field(kind, w, h, seed)


class Device:
    """One case's four input frames and an output on the device: uploaded once, whatever number of calls follows."""

    def __init__(self, ctx, prev, curr, fwd, bwd):
        h, w = prev.shape[:2]
        self.ctx = ctx
        self.p, self.c = ctx.frame_from(prev), ctx.frame_from(curr)
        self.f, self.b = ctx.frame_from(fwd, MV), ctx.frame_from(bwd, MV)
        self.o = ctx.create_frame(w, h)

    def run(self, t, match_sad, tolerance):
        self.ctx.interpolate_compensated_bidirectional(self.p, self.c, self.f, self.b, self.o, t, match_sad, tolerance)
        return self.ctx.download(self.o)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for f in (self.p, self.c, self.f, self.b, self.o):
            self.ctx.destroy_frame(f)


@pytest.mark.parametrize("kind", KINDS)
def test_every_pixel_equals_the_model(ctx, kind):
    for i, (w, h) in enumerate(SIZES):
        prev, curr, fwd, bwd = case(ctx, kind, w, h, 13 * i + 5)
        with Device(ctx, prev, curr, fwd, bwd) as dev:
            for t in bc.FACTORS:
                for ms in bc.MATCH:
                    for tol in bc.TOLERANCES:
                        got = dev.run(t, ms, tol)
                        want = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol)
                        assert (got == want).all(), f"{w}x{h} {kind} t={t} match_sad={ms} tolerance={tol}: {first_bad(got, want)}"
                        if t == 0.0:
                            assert (got == prev).all()                    # the header: t = 0 gives prev
                        if t == 1.0:
                            assert (got == curr).all()                    # ... and t = 1 curr


def test_shared_cases_equal_the_model(ctx):
    """The cases on which tests/test_bidir_model.py tells the model's mutants from it."""
    for name, prev, curr, fwd, bwd, ms, tols in bc.shared_cases():
        with Device(ctx, prev, curr, fwd, bwd) as dev:
            for tol in tols:
                for t in (0.25, 0.5, 0.3):
                    got = dev.run(t, ms, tol)
                    want = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol)
                    assert (got == want).all(), f"{name} t={t} tolerance={tol}: {first_bad(got, want)}"


def test_the_walk_reaches_16(ctx):
    """bc.walk_reach at tolerance 0: both projections land on one pixel of a key image of holes.  Byte for byte the model, and
    literally: the holes at distance 16 along an axis are filled from it, those at 17 are not."""
    prev, curr, fwd, bwd, blank = bc.walk_reach()
    ms = cases.WALK_REACH_MATCH_SAD
    with Device(ctx, prev, curr, fwd, bwd) as dev, Device(ctx, prev, curr, blank, blank) as dev_blank:
        for t in cases.WALK_REACH_FACTORS:
            got, got_blank = dev.run(t, ms, 0), dev_blank.run(t, ms, 0)
            for g, (f, b) in ((got, (fwd, bwd)), (got_blank, (blank, blank))):
                want = bd.interpolate_bidirectional(prev, curr, f, b, t, ms, 0)
                assert (g == want).all(), f"t={t}: {first_bad(g, want)}"
            cases.check_walk_reach(got, got_blank, t)


@pytest.mark.parametrize("kind", KINDS)
def test_motion_consistency_equals_the_model(ctx, kind):
    for i, (w, h) in enumerate(SIZES):
        _, _, fwd, bwd = case(ctx, kind, w, h, 13 * i + 5)
        f, b = ctx.frame_from(fwd, MV), ctx.frame_from(bwd, MV)
        pitch = w + 5                                                     # padded, and odd: rows on every byte alignment
        buf, mask = ctx.create_mask(w, h, pitch=pitch, fill=0x5A)
        try:
            for tol in bc.TOLERANCES:
                for (a, fa), (o, fo) in (((fwd, f), (bwd, b)), ((bwd, b), (fwd, f))):
                    ctx.motion_consistency(fa, fo, tol, mask)
                    rows, raw = ctx.download_mask(buf, mask)
                    assert (rows[:, w:] == 0x5A).all() and (raw[h * pitch:] == 0x5A).all()    # the padding keeps its fill
                    assert (rows[:, :w] == bd.consistency(a, o, tol)).all(), (kind, w, h, tol)
        finally:
            for x in (f, b, buf):
                ctx.destroy_frame(x)


def test_padded_pitches(ctx):
    w, h = 257, 131
    prev, curr, fwd, bwd = bc.field("small", w, h, 17)
    bp, p = pitched(ctx, prev, 3)
    bcur, c = pitched(ctx, curr, 5)
    bf, f = pitched(ctx, fwd, 7, MV)
    bb, b = pitched(ctx, bwd, 11, MV)
    bo, o = pitched(ctx, np.zeros((h, w, 4), np.uint8), 9)
    try:
        for t, ms, tol in [(0.5, 1020, 1), (0.25, 0, 0), (0.3, 48, 64), (1.0, 1020, 0), (0.0, 48, 1), (5.0 / 6.0, 48, 1)]:
            ctx.interpolate_compensated_bidirectional(p, c, f, b, o, t, ms, tol)
            raw = ctx.download(bo)
            assert (raw[:, w:] == 0x5A).all()                             # the padding is not written
            want = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol)
            assert (raw[:, :w] == want).all(), first_bad(raw[:, :w], want)
    finally:
        for x in (bp, bcur, bf, bb, bo):
            ctx.destroy_frame(x)


def test_multi_equals_single_calls(ctx):
    w, h = 200, 120
    prev, curr, fwd, bwd = bc.field("piecewise", w, h, 23)
    factors = [0.25, 0.5, 1.0, 0.5, 0.0, 0.3, 0.75]                       # a repeated factor among them
    with Device(ctx, prev, curr, fwd, bwd) as dev:
        outs = [ctx.create_frame(w, h) for _ in factors]
        try:
            ctx.interpolate_compensated_bidirectional_multi(dev.p, dev.c, dev.f, dev.b, outs, factors, 48, 1)
            for t, o in zip(factors, outs):
                got = ctx.download(o)
                assert (got == dev.run(t, 48, 1)).all(), t
                assert (got == bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, 48, 1)).all(), t
        finally:
            for o in outs:
                ctx.destroy_frame(o)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (96, 64), (200, 120), (130, 90), (96, 64), (300, 170)]
    inputs = [bc.field("small" if i % 2 else "piecewise", w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    alone = []
    for arrays in inputs:
        with Device(ctx, *arrays) as dev:
            alone.append(dev.run(0.75, 48, 1))

    def enqueue(i, prev, curr, fwd, bwd):
        h, w = prev.shape[:2]
        p, c, f, b = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(fwd, MV), ctx.frame_from(bwd, MV)
        o = ctx.create_frame(w, h)
        ctx.interpolate_compensated_bidirectional(p, c, f, b, o, 0.75, 48, 1)
        return p, c, f, b, o

    three_lanes(ctx, inputs, enqueue, alone)


@pytest.mark.parametrize("kind", KINDS)
def test_full_frame(ctx, kind):
    w, h = 640, 360
    prev, curr, fwd, bwd = case(ctx, kind, w, h, 3)
    with Device(ctx, prev, curr, fwd, bwd) as dev:
        for t, ms, tol in ((0.5, 48, 1), (0.3, 1020, 0), (0.25, 48, 64)):
            got = dev.run(t, ms, tol)
            want = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol)
            assert (got == want).all(), f"{kind} t={t}: {first_bad(got, want)}"


def test_rois_of_4k(ctx):
    w, h = 3840, 2160
    rng = np.random.default_rng(w)
    rois = [(0, 0, 64, 64), (w - 64, h - 64, 64, 64)] + [(int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64)), 64, 64)
                                                         for _ in range(6)]
    for kind, t, ms, tol in (("small", 0.3, 48, 1), ("random", 0.5, 1020, 64), ("motion", 0.25, 48, 0)):
        prev, curr, fwd, bwd = case(ctx, kind, w, h, 9)
        with Device(ctx, prev, curr, fwd, bwd) as dev:
            got = dev.run(t, ms, tol)
        for x, y, rw, rh in rois:
            want = bd.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol, roi=(x, y, rw, rh))
            assert (got[y:y + rh, x:x + rw] == want).all(), (kind, x, y)


def default_path(ctx, p, c, w, h):
    """lfg_interpolate_frames under the default settings, and motion + interpolate called one by one."""
    o, m = ctx.create_frame(w, h), ctx.create_frame(w, h, MV)
    try:
        ctx.interpolate_frames(p, c, o, 0.5)
        got = ctx.download(o)
        ctx.motion(p, c, m)
        ctx.interpolate(p, c, m, o, 0.5)
        return got, ctx.download(o)
    finally:
        ctx.destroy_frame(o)
        ctx.destroy_frame(m)


def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 40, 24
    prev, curr, fwd, bwd = bc.field("small", w, h, 1)
    p, c, f, b = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(fwd, MV), ctx.frame_from(bwd, MV)
    o, o2 = ctx.create_frame(w, h), ctx.create_frame(w, h)
    pattern = np.full((h, w, 4), 0x5A, np.uint8)
    ctx.upload(o, pattern)
    ctx.upload(o2, pattern)
    small = ctx.create_frame(w - 1, h)
    small_mv = ctx.create_frame(w, h - 1, MV)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)    # a pitch that is not a multiple of 4
    odd_mv = capi.Context.wrap(wide.data, w, h, MV, pitch=w * 2 + 1)                # ... of 2
    off_mv = capi.Context.wrap(wide.data + 1, w, h, MV, pitch=w * 2)                # a base that is not 2-byte aligned
    big = ctx.create_frame(w, h)
    mv_in_big = capi.Context.wrap(big.data, w, h, MV, pitch=w * 2)                  # vectors in the first half of `big`
    empty = capi.Frame()
    B = ctypes.byref

    def single(a, d, v, r, out, t=0.5, ms=48, tol=1):
        return lib.lfg_interpolate_compensated_bidirectional(ctx.h, a and B(a), d and B(d), v and B(v), r and B(r), out and B(out),
                                                             t, ms, tol)

    bad = [
        single(None, c, f, b, o), single(p, None, f, b, o), single(p, c, None, b, o), single(p, c, f, None, o),
        single(p, c, f, b, None), single(empty, c, f, b, o), single(p, c, f, empty, o),
        single(p, c, p, b, o), single(p, c, f, p, o),        # a field of the wrong format
        single(p, f, f, b, o),                               # curr of the wrong format
        single(p, c, f, b, small), single(p, c, small_mv, b, o), single(p, c, f, small_mv, o), single(small, c, f, b, o),
        single(odd, c, f, b, o), single(p, odd, f, b, o), single(p, c, odd_mv, b, o), single(p, c, f, odd_mv, o),
        single(p, c, off_mv, b, o), single(p, c, f, off_mv, o),
        single(p, c, f, b, p), single(p, c, f, b, c),        # the output overlaps an input
        single(p, c, mv_in_big, b, big), single(p, c, f, mv_in_big, big),
        single(p, c, f, b, o, float("nan")), single(p, c, f, b, o, float("inf")), single(p, c, f, b, o, -0.01),
        single(p, c, f, b, o, 1.01), single(p, c, f, b, o, 0.5, -1), single(p, c, f, b, o, 0.5, 1021),
        single(p, c, f, b, o, 0.5, 48, -1), single(p, c, f, b, o, 0.5, 48, 65),
    ]

    def multi(outs, factors, count=None, ms=48, tol=1):
        po = (capi._FP * len(outs))(*[ctypes.pointer(x) for x in outs])
        pf = (ctypes.c_float * len(factors))(*factors)
        return lib.lfg_interpolate_compensated_bidirectional_multi(ctx.h, B(p), B(c), B(f), B(b), po, pf,
                                                                   len(outs) if count is None else count, ms, tol)

    bad += [
        multi([o, o], [0.25, 0.5]),                          # two outputs alias each other
        multi([o], [0.5], count=0), multi([o] * 17, [0.5] * 17),
        multi([o, o2], [0.5, float("nan")]), multi([o, o2], [0.5, 1.01]), multi([o, o2], [0.5, 0.5], ms=2000),
        multi([o, o2], [0.5, 0.5], tol=65), multi([o, o2], [0.5, 0.5], tol=-1), multi([o, c], [0.5, 0.5]),
        lib.lfg_interpolate_compensated_bidirectional_multi(ctx.h, B(p), B(c), B(f), B(b), None, None, 1, 48, 1),
    ]

    # lfg_motion_consistency: the mask lies in an RGBA8 frame of 0x5A bytes, which must stay as it is
    def consistency(a, d, tol, m):
        return lib.lfg_motion_consistency(ctx.h, a and B(a), d and B(d), tol, m and B(m))

    mask = capi.Mask(o.data, w, h, w)
    bad += [
        consistency(None, b, 1, mask), consistency(f, None, 1, mask), consistency(f, b, 1, None), consistency(empty, b, 1, mask),
        consistency(p, b, 1, mask), consistency(f, p, 1, mask),                   # a frame that holds no vectors
        consistency(f, small_mv, 1, mask), consistency(small_mv, b, 1, mask),
        consistency(odd_mv, b, 1, mask), consistency(f, odd_mv, 1, mask), consistency(off_mv, b, 1, mask), consistency(f, off_mv, 1, mask),
        consistency(f, b, -1, mask), consistency(f, b, 65, mask),
        consistency(f, b, 1, capi.Mask(None, w, h, w)), consistency(f, b, 1, capi.Mask(o.data, w - 1, h, w)),
        consistency(f, b, 1, capi.Mask(o.data, w, h + 1, w)), consistency(f, b, 1, capi.Mask(o.data, w, h, w - 1)),
        consistency(f, b, 1, capi.Mask(f.data, w, h, w)), consistency(f, b, 1, capi.Mask(b.data, w, h, w)),     # overlaps a field
    ]
    assert all(rc == -1 for rc in bad), bad                               # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    # the setter: every illegal value is refused and changes nothing
    assert [lib.lfg_set_bidirectional(ctx.h, v) for v in (-2, 65, 1000, -100)] == [-1] * 4
    ctx.sync()
    assert (ctx.download(o) == pattern).all() and (ctx.download(o2) == pattern).all()
    got, want = default_path(ctx, p, c, w, h)
    assert (got == want).all()
    for x in (p, c, f, b, o, o2, small, small_mv, wide, big):
        ctx.destroy_frame(x)


# ---- lfg_set_bidirectional

FACTORS = [0.25, 0.5, 5.0 / 6.0]


def explicit(ctx, p, c, w, h, estimator, radius, factors, match_sad, tolerance):
    """The sequence the header gives for the switch, call by call: both estimates, both refinements, the bidirectional call."""
    fs = [ctx.create_frame(w, h, MV) for _ in range(4)]
    outs = [ctx.create_frame(w, h) for _ in factors]
    try:
        for (a, d), m in (((p, c), fs[0]), ((c, p), fs[1])):
            if estimator == "full":
                ctx.motion(a, d, m)
            else:
                ctx.motion_pyramid(a, d, m, 2, 16, 2)
        fwd, bwd = fs[0], fs[1]
        if radius >= 0:
            ctx.motion_refine(p, c, fs[0], fs[2], radius)
            ctx.motion_refine(c, p, fs[1], fs[3], radius)
            fwd, bwd = fs[2], fs[3]
        ctx.interpolate_compensated_bidirectional_multi(p, c, fwd, bwd, outs, factors, match_sad, tolerance)
        return [ctx.download(o) for o in outs]
    finally:
        for x in fs + outs:
            ctx.destroy_frame(x)


def through_frames(ctx, p, c, w, h, factors):
    """lfg_interpolate_frames for the first factor and lfg_interpolate_frames_multi for all: (single, [multi])."""
    outs = [ctx.create_frame(w, h) for _ in factors]
    try:
        ctx.interpolate_frames(p, c, outs[0], factors[0])
        single = ctx.download(outs[0])
        ctx.interpolate_frames_multi(p, c, outs, factors)
        return single, [ctx.download(o) for o in outs]
    finally:
        for o in outs:
            ctx.destroy_frame(o)


@pytest.mark.parametrize("estimator", ["full", "pyramid"])
@pytest.mark.parametrize("radius", [-1, 1])
def test_the_switch_equals_the_explicit_calls(ctx, estimator, radius):
    prev, curr = cases.matrix_scene()
    h, w = prev.shape[:2]
    setting = (estimator, radius, "compensated", capi.SEMANTICS_INTENDED)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    try:
        apply(ctx, setting)
        _, off = through_frames(ctx, p, c, w, h, FACTORS)
        want = explicit(ctx, p, c, w, h, estimator, radius, FACTORS, capi.DEFAULT_MATCH_SAD, 1)
        ctx.set_bidirectional(1)
        single, multi = through_frames(ctx, p, c, w, h, FACTORS)
        assert (single == want[0]).all(), first_bad(single, want[0])
        for t, g, e in zip(FACTORS, multi, want):
            assert (g == e).all(), f"t={t}: {first_bad(g, e)}"
        assert any(not (g == e).all() for g, e in zip(multi, off))        # the route is not the one-field one
        # cut detection runs on fwd as before: a correlated pair is no cut and the bytes stay
        ctx.set_cut_detection(200)
        single, multi = through_frames(ctx, p, c, w, h, FACTORS)
        assert not ctx.last_pair_stats()[1]
        assert (single == want[0]).all() and all((g == e).all() for g, e in zip(multi, want))
        ctx.set_cut_detection(-1)
        # an illegal value is refused and the setting stays
        assert ctx.lib.lfg_set_bidirectional(ctx.h, 65) == -1
        assert (through_frames(ctx, p, c, w, h, FACTORS)[0] == want[0]).all()
        # another tolerance is another call
        ctx.set_bidirectional(0)
        zero = explicit(ctx, p, c, w, h, estimator, radius, FACTORS, capi.DEFAULT_MATCH_SAD, 0)
        assert all((g == e).all() for g, e in zip(through_frames(ctx, p, c, w, h, FACTORS)[1], zero))
        # back at -1: today's bytes
        ctx.set_bidirectional(-1)
        single, multi = through_frames(ctx, p, c, w, h, FACTORS)
        assert (single == off[0]).all() and all((g == e).all() for g, e in zip(multi, off))
    finally:
        ctx.set_bidirectional(-1)
        apply(ctx, DEFAULT)
        ctx.destroy_frame(p)
        ctx.destroy_frame(c)


@pytest.mark.parametrize("where", ["static protection", "extrapolation", "shader", "shader, reference semantics"])
def test_the_switch_has_no_effect(ctx, where):
    prev, curr = cases.matrix_scene()
    h, w = prev.shape[:2]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    try:
        apply(ctx, ("full", -1, "shader", capi.SEMANTICS_REFERENCE if "reference" in where else capi.SEMANTICS_INTENDED)
              if "shader" in where else COMPENSATED)
        if where == "static protection":
            ctx.set_static_protection(8)
        if where == "extrapolation":
            ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
        single, multi = through_frames(ctx, p, c, w, h, FACTORS)
        ctx.set_bidirectional(1)
        again, again_multi = through_frames(ctx, p, c, w, h, FACTORS)
        assert (single == again).all() and all((g == e).all() for g, e in zip(again_multi, multi))
    finally:
        ctx.set_bidirectional(-1)
        ctx.set_static_protection(-1)
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        apply(ctx, DEFAULT)
        ctx.destroy_frame(p)
        ctx.destroy_frame(c)


def test_the_switch_follows_a_change_of_size(ctx):
    """The backward temporaries are made again with the frame size, as the forward ones are."""
    try:
        apply(ctx, ("pyramid", 1, "compensated", capi.SEMANTICS_INTENDED))
        ctx.set_bidirectional(1)
        for w, h, seed in ((96, 64, 1), (33, 17, 2), (200, 120, 3), (96, 64, 4)):
            prev, curr = cases.small_scene(w, h, seed)
            p, c = ctx.frame_from(prev), ctx.frame_from(curr)
            try:
                want = explicit(ctx, p, c, w, h, "pyramid", 1, [0.5], capi.DEFAULT_MATCH_SAD, 1)[0]
                got = through_frames(ctx, p, c, w, h, [0.5])[0]
                assert (got == want).all(), (w, h, first_bad(got, want))
            finally:
                ctx.destroy_frame(p)
                ctx.destroy_frame(c)
    finally:
        ctx.set_bidirectional(-1)
        apply(ctx, DEFAULT)


# ---- lfg_host --bidirectional

def test_host_bidirectional_stream_matches_capi(tmp_path):
    w, h, n = 1920, 1080, 3
    frames = [synth.make_prev(w, h)]
    for k in range(1, n):
        frames.append(synth.translate(frames[-1], (12, -6), synth.BASE_SEED + k))
    info, got = host_run(tmp_path, frames, (w, h), "--semantics", "intended", "--interpolator", "compensated", "--bidirectional", "1")
    assert len(got) == 2 * n - 1 and info["bidirectional"] == 1
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ins = [c.frame_from(f) for f in frames]
        ups = [c.create_frame(w, h) for _ in frames]
        for i, u in zip(ins, ups):
            c.scale(i, u)
        f, b = c.create_frame(w, h, MV), c.create_frame(w, h, MV)
        o = c.create_frame(w, h)
        want = [c.download(ups[0])]
        for k in range(1, n):
            c.motion(ups[k - 1], ups[k], f)
            c.motion(ups[k], ups[k - 1], b)
            c.interpolate_compensated_bidirectional(ups[k - 1], ups[k], f, b, o, 0.5, 48, 1)
            want += [c.download(o), c.download(ups[k])]
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k
