"""lfg_frame_halve and lfg_motion_expand on the GPU against the CPU model (tests/expand_model.py), byte for byte; the named
cases of tests/expand_cases.py; pitches and views; lanes; argument checks; the half-resolution switch of
lfg_interpolate_frames[_multi] against the explicit sequence of public calls and against the CPU chain; the host's
--half-res-motion."""
import ctypes
import itertools

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import expand_cases as xc
from tests import expand_model as xm
from tests import pyramid_model as pm
from tests.gpu_kit import ESTIMATOR, INTERPOLATOR, ctx, first_bad, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (3, 3), (17, 9), (33, 17), (96, 64), (257, 131)]
RADII = [0, 1, 2]
FIELDS = ["uniform", "full", "pyramid", "random"]
MV = capi.FORMAT_MV_S8X2


def destroy(ctx, *frames):
    for f in frames:
        ctx.destroy_frame(f)


def run_halve(ctx, img):
    h, w = img.shape[:2]
    i, o = ctx.frame_from(img), ctx.create_frame(*xm.low_size(w, h))
    try:
        ctx.frame_halve(i, o)
        return ctx.download(o)
    finally:
        destroy(ctx, i, o)


def run_expand(ctx, prev, curr, low, radius):
    h, w = prev.shape[:2]
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(low, MV)
    o = ctx.create_frame(w, h, MV)
    try:
        ctx.motion_expand(p, c, m, o, radius)
        return ctx.download(o)
    finally:
        destroy(ctx, p, c, m, o)


def estimate_low(ctx, prev, curr, estimator):
    """The half-size field as the switch makes it: both frames halved on the GPU, then lfg_motion(8, 16) or
    lfg_motion_pyramid(1, 16, 2) on the halves, under the context's semantics."""
    h, w = prev.shape[:2]
    wl, hl = xm.low_size(w, h)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    hp, hc, m = ctx.create_frame(wl, hl), ctx.create_frame(wl, hl), ctx.create_frame(wl, hl, MV)
    try:
        ctx.frame_halve(p, hp)
        ctx.frame_halve(c, hc)
        if estimator == "full":
            ctx.motion(hp, hc, m)
        else:
            ctx.motion_pyramid(hp, hc, m, 1, 16, 2)
        return ctx.download(m)
    finally:
        destroy(ctx, p, c, hp, hc, m)


def case(ctx, field, w, h, seed):
    """(prev, curr, mv_low int8) for one kind of coarse field."""
    rng = np.random.default_rng(seed)
    wl, hl = xm.low_size(w, h)
    if field in ("full", "pyramid"):
        prev, curr = cases.small_scene(w, h, seed)
        return prev, curr, estimate_low(ctx, prev, curr, field)
    prev = cases.textured(w, h, seed)
    low = np.zeros((hl, wl, 2), np.int8)
    if field == "uniform":                # an odd true vector under a uniform coarse one: the parity step at every pixel
        low[...] = rng.integers(-10, 11, 2)
        true = 2 * low[0, 0].astype(int) + rng.integers(-1, 2, 2)
        curr = synth.translate(prev, tuple(-int(v) for v in true), synth.BASE_SEED + seed)
    else:                                 # dense random over the full byte range, -128 and 127 among them
        low = rng.integers(-128, 128, (hl, wl, 2)).astype(np.int8)
        low.reshape(-1)[:2] = (-128, 127)
        curr = np.clip(prev.astype(np.int16) + rng.integers(-40, 41, prev.shape), 0, 255).astype(np.uint8)
    return prev, curr, low


@pytest.mark.parametrize("w,h", SIZES + [(640, 360)])
def test_halve_equals_the_model(ctx, w, h):
    img = cases.textured(w, h, 7 * w + h)
    want = xm.halve(img)
    got = run_halve(ctx, img)
    assert (got == want).all(), first_bad(got, want)
    assert (got == pm.reduce(img)).all()


@pytest.mark.parametrize("field", FIELDS)
def test_every_vector_equals_the_model(ctx, field):
    for i, (w, h) in enumerate(SIZES):
        prev, curr, low = case(ctx, field, w, h, 13 * i + 5)
        for radius in RADII:
            got = run_expand(ctx, prev, curr, low, radius)
            want = xm.expand(prev, curr, low, radius)
            assert (got == want).all(), f"{w}x{h} {field} radius={radius}: {first_bad(got, want)}"
            assert got.min() >= -127


@pytest.mark.parametrize("field", ["pyramid", "random"])
def test_one_whole_640x360_frame(ctx, field):
    prev, curr, low = case(ctx, field, 640, 360, 3)
    for radius in RADII:
        got = run_expand(ctx, prev, curr, low, radius)
        want = xm.expand(prev, curr, low, radius)
        assert (got == want).all(), f"{field} radius={radius}: {first_bad(got, want)}"


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_named_cases(ctx, name):
    prev, curr, low, (x, y), want, _ = xc.CASES[name]()
    for radius in RADII:
        got = run_expand(ctx, prev, curr, low, radius)
        model = xm.expand(prev, curr, low, radius)
        assert (got == model).all(), f"{name} radius={radius}: {first_bad(got, model)}"
        assert tuple(int(c) for c in got[y, x]) == want, (name, radius)


def test_padded_pitches_and_views(ctx):
    """All four frames of lfg_motion_expand, and both of lfg_frame_halve, as views into wider frames (lfg_frame_wrap) with
    pitches of their own; the padding is not written."""
    w, h = 257, 131
    wl, hl = xm.low_size(w, h)
    prev, curr, low = case(ctx, "random", w, h, 17)
    bp, p = pitched(ctx, prev, 3)
    bc, c = pitched(ctx, curr, 5)
    bm, m = pitched(ctx, low, 7, MV)
    bo, o = pitched(ctx, np.zeros((h, w, 2), np.int8), 9, MV)
    bh, hv = pitched(ctx, np.zeros((hl, wl, 4), np.uint8), 11)
    try:
        for radius in RADII:
            ctx.motion_expand(p, c, m, o, radius)
            raw = ctx.download(bo)
            assert (raw[:, w:].view(np.uint8) == 0x5A).all()
            want = xm.expand(prev, curr, low, radius)
            assert (raw[:, :w] == want).all(), first_bad(raw[:, :w], want)
        ctx.frame_halve(p, hv)
        raw = ctx.download(bh)
        assert (raw[:, wl:] == 0x5A).all()
        assert (raw[:, :wl] == xm.halve(prev)).all()
    finally:
        destroy(ctx, bp, bc, bm, bo, bh)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (97, 65), (200, 120), (131, 90), (97, 65), (300, 170)]
    inputs = [case(ctx, "random" if i % 2 else "uniform", w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    alone = [run_expand(ctx, a, b, v, i % 3) for i, (a, b, v) in enumerate(inputs)]
    for (a, b, v), got, i in zip(inputs, alone, range(len(inputs))):
        assert (got == xm.expand(a, b, v, i % 3)).all()

    def enqueue(i, a, b, v):
        h, w = a.shape[:2]
        p, c, m = ctx.frame_from(a), ctx.frame_from(b), ctx.frame_from(v, MV)
        o = ctx.create_frame(w, h, MV)
        ctx.motion_expand(p, c, m, o, i % 3)
        return p, c, m, o

    three_lanes(ctx, inputs, enqueue, alone)


def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 41, 25
    wl, hl = xm.low_size(w, h)
    prev, curr, low = case(ctx, "random", w, h, 1)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(low, MV)
    o = ctx.create_frame(w, h, MV)
    pattern = np.full((h, w, 2), 0x5A, np.int8)
    ctx.upload(o, pattern)
    half = ctx.create_frame(wl, hl)
    half_pattern = np.full((hl, wl, 4), 0x5A, np.uint8)
    ctx.upload(half, half_pattern)
    small = ctx.create_frame(w - 1, h)
    small_mv = ctx.create_frame(w, h - 1, MV)
    full_size_low = ctx.create_frame(w, h, MV)                   # mv_low of the frames' own size
    floor_low = ctx.create_frame(w // 2, hl, MV)                 # floor(W / 2) instead of ceil
    floor_half = ctx.create_frame(w // 2, hl)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)              # pitch not a multiple of 4
    shifted = capi.Context.wrap(wide.data + 2, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 4)      # data not 4-byte aligned
    wide_mv = ctx.create_frame(w + 1, h, MV)
    odd_mv = capi.Context.wrap(wide_mv.data, w, h, MV, pitch=w * 2 + 1)                        # pitch not a multiple of 2
    shifted_mv = capi.Context.wrap(wide_mv.data + 1, w, h, MV, pitch=w * 2 + 2)                # data not 2-byte aligned
    odd_low = capi.Context.wrap(wide_mv.data, wl, hl, MV, pitch=wl * 2 + 1)
    big = ctx.create_frame(w, h)
    mv_in_big = capi.Context.wrap(big.data, w, h, MV, pitch=w * 2)                             # vectors inside `big`'s bytes
    low_in_out = capi.Context.wrap(o.data, wl, hl, MV, pitch=wl * 2)                           # mv_low inside mv_out's bytes
    half_in_p = capi.Context.wrap(p.data, wl, hl, capi.FORMAT_RGBA8, pitch=w * 4)              # out inside in's bytes
    odd_half = capi.Context.wrap(wide.data, wl, hl, capi.FORMAT_RGBA8, pitch=wl * 4 + 2)
    empty = capi.Frame()
    B = ctypes.byref

    def expand(a, b, lo, vo, radius=1):
        return lib.lfg_motion_expand(ctx.h, a and B(a), b and B(b), lo and B(lo), vo and B(vo), radius)

    def halve(a, b):
        return lib.lfg_frame_halve(ctx.h, a and B(a), b and B(b))

    bad = [
        expand(None, c, m, o), expand(p, None, m, o), expand(p, c, None, o), expand(p, c, m, None), expand(empty, c, m, o),
        expand(p, c, half, o), expand(p, m, m, o), expand(m, c, m, o), expand(p, c, m, p),                  # wrong formats
        expand(small, c, m, o), expand(p, small, m, o), expand(p, c, m, small_mv),                          # wrong sizes
        expand(p, c, full_size_low, o), expand(p, c, floor_low, o), expand(p, c, o, o),                     # wrong mv_low sizes
        expand(odd, c, m, o), expand(p, odd, m, o), expand(shifted, c, m, o), expand(p, c, odd_low, o),
        expand(p, c, m, odd_mv), expand(p, c, m, shifted_mv),
        expand(p, c, low_in_out, o), expand(big, c, m, mv_in_big), expand(p, big, m, mv_in_big),            # overlaps
        expand(p, c, m, o, -1), expand(p, c, m, o, 3), expand(p, c, m, o, 1000),
        halve(None, half), halve(p, None), halve(empty, half), halve(m, half), halve(p, m),                 # NULL, empty, formats
        halve(p, floor_half), halve(p, big), halve(small, half),                                            # wrong out sizes
        halve(odd, half), halve(shifted, half), halve(p, odd_half), halve(p, half_in_p),                    # alignment, overlap
    ]
    assert all(rc == -1 for rc in bad), bad                          # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_set_half_resolution_motion(ctx.h, -2) == -1
    assert lib.lfg_set_half_resolution_motion(ctx.h, 3) == -1
    assert "lfg_set_half_resolution_motion" in lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert (ctx.download(o) == pattern).all()
    assert (ctx.download(half) == half_pattern).all()
    assert (ctx.download(m) == low).all() and (ctx.download(p) == prev).all()
    destroy(ctx, p, c, m, o, half, small, small_mv, full_size_low, floor_low, floor_half, wide, wide_mv, big)


# ---- the switch of lfg_interpolate_frames[_multi]

FACTORS = [0.25, 0.5, 0.9]
SWITCH = list(itertools.product(("full", "pyramid"), (-1, 1), ("shader", "compensated"), (-1, 1)))


class Pair:
    """A pair on the device, with every frame the explicit sequence needs."""

    def __init__(self, ctx, prev, curr):
        self.ctx, (self.h, self.w) = ctx, prev.shape[:2]
        w, h, (wl, hl) = self.w, self.h, xm.low_size(self.w, self.h)
        self.p, self.c = ctx.frame_from(prev), ctx.frame_from(curr)
        self.hp, self.hc, self.low = ctx.create_frame(wl, hl), ctx.create_frame(wl, hl), ctx.create_frame(wl, hl, MV)
        self.mv = [ctx.create_frame(w, h, MV) for _ in range(4)]
        self.outs = [ctx.create_frame(w, h) for _ in FACTORS]
        self.ref = ctx.create_frame(w, h)

    def close(self):
        destroy(self.ctx, self.p, self.c, self.hp, self.hc, self.low, self.ref, *self.mv, *self.outs)

    def vectors(self, a, b, estimator, refine, expand_radius, est, refined):
        """The public calls that the switch stands for, for the pair (a, b): the field the interpolator takes."""
        ctx = self.ctx
        ctx.frame_halve(a, self.hp)
        ctx.frame_halve(b, self.hc)
        if estimator == "full":
            ctx.motion(self.hp, self.hc, self.low)
        else:
            ctx.motion_pyramid(self.hp, self.hc, self.low, 1, 16, 2)
        ctx.motion_expand(a, b, self.low, est, expand_radius)
        if refine < 0:
            return est
        ctx.motion_refine(a, b, est, refined, refine)
        return refined

    def explicit(self, setting, expand_radius, t):
        """One generated frame by the explicit sequence, downloaded."""
        estimator, refine, interpolator, bidir = setting
        ctx = self.ctx
        fwd = self.vectors(self.p, self.c, estimator, refine, expand_radius, self.mv[0], self.mv[1])
        if interpolator == "shader":
            ctx.interpolate(self.p, self.c, fwd, self.ref, t)
        elif bidir < 0:
            ctx.interpolate_compensated(self.p, self.c, fwd, self.ref, t, 48)
        else:
            bwd = self.vectors(self.c, self.p, estimator, refine, expand_radius, self.mv[2], self.mv[3])
            ctx.interpolate_compensated_bidirectional(self.p, self.c, fwd, bwd, self.ref, t, 48, bidir)
        return ctx.download(self.ref)


def select(ctx, setting, expand_radius):
    estimator, refine, interpolator, bidir = setting
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    ctx.set_motion_estimator(ESTIMATOR[estimator])
    ctx.set_vector_refinement(refine)
    ctx.set_interpolator(INTERPOLATOR[interpolator], 48)
    ctx.set_bidirectional(bidir)
    ctx.set_half_resolution_motion(expand_radius)


def deselect(ctx):
    select(ctx, ("full", -1, "shader", -1), -1)
    ctx.set_semantics(capi.SEMANTICS_REFERENCE)
    ctx.set_fused_motion_interpolate(False)


@pytest.fixture(scope="module")
def matrix_pair(ctx):
    prev, curr = cases.matrix_scene()
    pair = Pair(ctx, prev, curr)
    pair.host = (prev, curr)
    yield pair
    pair.close()


@pytest.mark.parametrize("setting", SWITCH, ids=lambda s: "-".join(str(v) for v in s))
def test_switch_equals_the_explicit_sequence(ctx, matrix_pair, setting):
    pair = matrix_pair
    try:
        for expand_radius in (1, 2) if setting == SWITCH[0] else (1,):
            select(ctx, setting, expand_radius)
            want = [pair.explicit(setting, expand_radius, t) for t in FACTORS]
            for fused in (False, True):                                   # the fused order does not apply while the switch is on
                ctx.set_fused_motion_interpolate(fused)
                ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], FACTORS[0])
                got = ctx.download(pair.outs[0])
                assert (got == want[0]).all(), (setting, expand_radius, fused, first_bad(got, want[0]))
            ctx.set_fused_motion_interpolate(False)
            ctx.interpolate_frames_multi(pair.p, pair.c, pair.outs, FACTORS)
            for t, o, e in zip(FACTORS, pair.outs, want):
                got = ctx.download(o)
                assert (got == e).all(), (setting, expand_radius, t, first_bad(got, e))
    finally:
        deselect(ctx)


@pytest.mark.parametrize("setting", [("pyramid", 1, "compensated", 1), ("full", -1, "shader", 1)], ids=lambda s: "-".join(str(v) for v in s))
def test_switch_equals_the_cpu_chain(ctx, matrix_pair, setting):
    """cases.Chain with the model's field in the estimator's place: the halves, the estimator's model on them, the expansion."""
    import oracle
    estimator, refine, interpolator, semantics = setting
    prev, curr = matrix_pair.host
    hp, hc = xm.halve(prev), xm.halve(curr)
    low = pm.motion_pyramid(hp, hc, 1, 16, 2) if estimator == "pyramid" else oracle.motion(hp, hc, semantics=semantics).astype(np.int8)
    chain = cases.Chain(prev, curr)
    chain._estimated[(estimator, semantics if estimator == "full" else None)] = xm.expand(prev, curr, low, 1)
    want = chain.frames(setting, FACTORS)
    try:
        select(ctx, (estimator, refine, interpolator, -1), 1)
        ctx.interpolate_frames_multi(matrix_pair.p, matrix_pair.c, matrix_pair.outs, FACTORS)
        for t, o, e in zip(FACTORS, matrix_pair.outs, want):
            got = ctx.download(o)
            assert (got == e).all(), (setting, t, first_bad(got, e))
    finally:
        deselect(ctx)


def test_temporaries_follow_a_change_of_size(ctx):
    setting = ("pyramid", 1, "compensated", 1)
    try:
        for i, (w, h) in enumerate([(96, 64), (33, 17), (1, 1), (97, 64), (96, 64)]):
            pair = Pair(ctx, *cases.small_scene(w, h, 40 + i))
            try:
                select(ctx, setting, 1)
                want = pair.explicit(setting, 1, 0.5)
                ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], 0.5)
                got = ctx.download(pair.outs[0])
                assert (got == want).all(), (w, h, first_bad(got, want))
            finally:
                pair.close()
    finally:
        deselect(ctx)


def test_off_restores_the_bytes_and_an_invalid_value_leaves_the_setting(ctx, matrix_pair):
    pair = matrix_pair
    setting = ("pyramid", -1, "compensated", -1)

    def frame():
        ctx.interpolate_frames(pair.p, pair.c, pair.outs[0], 0.5)
        return ctx.download(pair.outs[0])

    try:
        select(ctx, setting, -1)
        before = frame()
        ctx.set_half_resolution_motion(1)
        on = frame()
        assert (on == pair.explicit(setting, 1, 0.5)).all()
        assert (on != before).any()                                      # the route changes the field on this scene
        assert ctx.lib.lfg_set_half_resolution_motion(ctx.h, 3) == -1    # refused: still radius 1
        assert (frame() == on).all()
        ctx.set_half_resolution_motion(-1)
        assert (frame() == before).all()
        assert ctx.lib.lfg_set_half_resolution_motion(ctx.h, -2) == -1   # refused: still off
        assert (frame() == before).all()
    finally:
        deselect(ctx)


# ---- the host

def test_host_half_resolution_stream_matches_capi(tmp_path):
    w, h, n = 1920, 1080, 3
    frames = [synth.make_prev(w, h)]
    for k in range(1, n):
        frames.append(synth.translate(frames[-1], (12, -6), synth.BASE_SEED + k))
    info, got = host_run(tmp_path, frames, (w, h), "--motion", "pyramid", "--interpolator", "compensated", "--semantics", "intended",
                         "--half-res-motion", "1")
    assert info["half_res_motion"] == 1
    assert len(got) == 2 * n - 1
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ins = [c.frame_from(f) for f in frames]
        ups = [c.create_frame(w, h) for _ in frames]
        for i, u in zip(ins, ups):
            c.scale(i, u)
        wl, hl = xm.low_size(w, h)
        hp, hc, low = c.create_frame(wl, hl), c.create_frame(wl, hl), c.create_frame(wl, hl, MV)
        m = c.create_frame(w, h, MV)
        o = c.create_frame(w, h)
        want = [c.download(ups[0])]
        for k in range(1, n):
            c.frame_halve(ups[k - 1], hp)
            c.frame_halve(ups[k], hc)
            c.motion_pyramid(hp, hc, low, 1, 16, 2)
            c.motion_expand(ups[k - 1], ups[k], low, m, 1)
            c.interpolate_compensated(ups[k - 1], ups[k], m, o, 0.5, 48)
            want += [c.download(o), c.download(ups[k])]
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k
