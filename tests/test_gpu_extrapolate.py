"""lfg_extrapolate_compensated on the GPU against the CPU model (tests/extrapolate_model.py), byte for byte; the generation
switch of lfg_interpolate_frames[_multi] against the CPU chain of the same stages; argument checks; lanes; the host's
--generation option, its presentation order and its --evaluate route."""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import extrapolate_cases as xc
from tests import extrapolate_model as ex
from tests.gpu_kit import DEFAULT, HOST, apply, ctx, first_bad, gpu_vectors, host_run, pitched, three_lanes
from tests.test_diff_model import INT_KEYS

pytestmark = pytest.mark.gpu

# one pixel, ragged, not a multiple of the 64 x 4 workgroup, exactly one workgroup column, several with a remainder
SIZES = [(1, 1), (7, 5), (33, 17), (64, 64), (257, 131)]
COMPENSATED = ("full", -1, "compensated", capi.SEMANTICS_INTENDED)


def case(ctx, field, w, h, seed):
    """(prev, curr, mv int8) for one kind of vector field: an estimator's on the GPU, or one of cases.field."""
    if field in ("motion", "pyramid"):
        prev = synth.make_prev(w, h, synth.BASE_SEED + seed)
        curr = synth.translate(prev, (5, -3) if field == "motion" else (-30, 18), synth.BASE_SEED + seed)
        return prev, curr, gpu_vectors(ctx, prev, curr, "full" if field == "motion" else "pyramid")
    return cases.field(field, w, h, seed)


def run(ctx, prev, curr, mv, a, match_sad):
    h, w = prev.shape[:2]
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o = ctx.create_frame(w, h)
    try:
        ctx.extrapolate_compensated(p, c, m, o, a, match_sad)
        return ctx.download(o)
    finally:
        for f in (p, c, m, o):
            ctx.destroy_frame(f)


@pytest.mark.parametrize("field", ["uniform", "piecewise", "random", "motion", "pyramid"])
def test_every_pixel_equals_the_model(ctx, field):
    for i, (w, h) in enumerate(SIZES):
        prev, curr, mv = case(ctx, field, w, h, 13 * i + 5)
        for a in xc.FACTORS:
            for ms in xc.MATCH:
                got = run(ctx, prev, curr, mv, a, ms)
                want = ex.extrapolate(prev, curr, mv, a, ms)
                assert (got == want).all(), f"{w}x{h} {field} a={a} match_sad={ms}: {first_bad(got, want)}"
                if a == 0.0:
                    assert (got == curr).all()                            # the header: a = 0 gives curr


def test_shared_cases_equal_the_model(ctx):
    """The cases whose power tests/test_extrapolate_model.py confirms, and on which it tells the model's mutants from it."""
    for name, prev, curr, mv, ms in xc.shared_cases():
        for a in xc.FACTORS:
            got = run(ctx, prev, curr, mv, a, ms)
            want = ex.extrapolate(prev, curr, mv, a, ms)
            assert (got == want).all(), f"{name} a={a}: {first_bad(got, want)}"


def test_full_frame(ctx):
    w, h = 640, 360
    for field, a, ms in (("piecewise", 0.5, 1020), ("random", 1.0 / 3.0, 48), ("random", 0.75, 1020), ("motion", 1.0, 48),
                         ("pyramid", 0.25, 48)):
        prev, curr, mv = case(ctx, field, w, h, 3)
        got = run(ctx, prev, curr, mv, a, ms)
        want = ex.extrapolate(prev, curr, mv, a, ms)
        assert (got == want).all(), f"{field} a={a}: {first_bad(got, want)}"


def test_rois_of_4k(ctx):
    w, h = 3840, 2160
    rng = np.random.default_rng(w)
    rois = [(0, 0, 64, 64), (w - 64, h - 64, 64, 64)] + [(int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64)), 64, 64)
                                                         for _ in range(6)]
    for field, a, ms in (("random", 1.0 / 3.0, 1020), ("motion", 1.0, 48)):
        prev, curr, mv = case(ctx, field, w, h, 9)
        got = run(ctx, prev, curr, mv, a, ms)
        for x, y, rw, rh in rois:
            want = ex.extrapolate(prev, curr, mv, a, ms, roi=(x, y, rw, rh))
            assert (got[y:y + rh, x:x + rw] == want).all(), (field, x, y)


def test_padded_and_odd_pitches(ctx):
    w, h = 257, 131
    prev, curr, mv = case(ctx, "random", w, h, 17)
    bp, p = pitched(ctx, prev, 3)
    bc, c = pitched(ctx, curr, 5)
    bm, m = pitched(ctx, mv, 7, capi.FORMAT_MV_S8X2)
    bo, o = pitched(ctx, np.zeros((h, w, 4), np.uint8), 9)
    try:
        for a, ms in [(0.5, 1020), (0.25, 0), (1.0 / 3.0, 48), (1.0, 1020), (0.0, 48)]:
            ctx.extrapolate_compensated(p, c, m, o, a, ms)
            raw = ctx.download(bo)
            assert (raw[:, w:] == 0x5A).all()                     # the padding is not written
            want = ex.extrapolate(prev, curr, mv, a, ms)
            assert (raw[:, :w] == want).all(), first_bad(raw[:, :w], want)
    finally:
        for f in (bp, bc, bm, bo):
            ctx.destroy_frame(f)


def test_multi_equals_single_calls(ctx):
    w, h = 200, 120
    prev, curr, mv = case(ctx, "piecewise", w, h, 23)
    aheads = [0.25, 0.5, 1.0, 0.5, 0.0, 1.0 / 3.0, 0.75]          # a repeated factor among them
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    outs = [ctx.create_frame(w, h) for _ in aheads]
    single = ctx.create_frame(w, h)
    try:
        ctx.extrapolate_compensated_multi(p, c, m, outs, aheads, 48)
        for a, o in zip(aheads, outs):
            got = ctx.download(o)
            ctx.extrapolate_compensated(p, c, m, single, a, 48)
            assert (got == ctx.download(single)).all(), a
            assert (got == ex.extrapolate(prev, curr, mv, a, 48)).all(), a
    finally:
        for f in [p, c, m, single] + outs:
            ctx.destroy_frame(f)


def test_hand_made_key_cases(ctx):
    """tests/extrapolate_cases.py: tie_collision_foreground, through the public call, with the literal values its docstring
    states: two sources collide on one destination, a hole has equal triples left and right, and the hole's c is foreground."""
    prev, curr, mv = xc.tie_collision_foreground()
    got = run(ctx, prev, curr, mv, 1.0, 1020)
    assert (got == ex.extrapolate(prev, curr, mv, 1.0, 1020)).all()
    assert (got[1, 6:9] == curr[3, 6:9]).all()                    # the longer vector won the collision
    assert (got[3, 6:9] == curr[3, 9]).all()                      # the +x donor, not the -x one: curr(5, 3) differs
    assert not (curr[3, 9] == curr[3, 5]).all()
    untouched = np.ones(got.shape[:2], bool)
    untouched[1, 6:9] = untouched[3, 6:9] = False
    assert (got[untouched] == curr[untouched]).all()
    got = run(ctx, prev, curr, mv, 0.5, 1020)                     # they land on row 2
    assert (got[2, 6:9] == curr[3, 6:9]).all() and (got[3, 6:9] == curr[3, 9]).all()


def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 40, 24
    prev, curr, mv = cases.field("random", w, h, 1)
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

    def single(a, b, v, out, ahead=0.5, ms=48):
        return lib.lfg_extrapolate_compensated(ctx.h, a and B(a), b and B(b), v and B(v), out and B(out), ahead, ms)

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

    def multi(outs, aheads, count=None, ms=48):
        po = (capi._FP * len(outs))(*[ctypes.pointer(f) for f in outs])
        pf = (ctypes.c_float * len(aheads))(*aheads)
        return lib.lfg_extrapolate_compensated_multi(ctx.h, B(p), B(c), B(m), po, pf, len(outs) if count is None else count, ms)

    bad += [
        multi([o, o], [0.25, 0.5]),              # two outputs alias each other
        multi([o], [0.5], count=0), multi([o] * 17, [0.5] * 17),
        multi([o, o2], [0.5, float("nan")]), multi([o, o2], [0.5, 1.01]), multi([o, o2], [0.5, 0.5], ms=2000),
        multi([o, c], [0.5, 0.5]),
    ]
    assert all(rc == -1 for rc in bad), bad                          # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_set_generation(ctx.h, 2) == -1 and lib.lfg_set_generation(ctx.h, -1) == -1
    ctx.sync()
    assert (ctx.download(o) == pattern).all() and (ctx.download(o2) == pattern).all()
    for f in (p, c, m, o, o2, small, small_mv, wide, big):
        ctx.destroy_frame(f)


# ---- lfg_set_generation

@pytest.fixture(scope="module")
def chain():
    prev, curr = cases.matrix_scene()
    return cases.Chain(prev, curr)


AHEADS = [0.5, 1.0, 1.0 / 3.0]


@pytest.mark.parametrize("estimator", ["full", "pyramid"])
@pytest.mark.parametrize("radius", [-1, 1])
def test_generation_switch_equals_the_chain(ctx, chain, estimator, radius):
    prev, curr = chain.prev, chain.curr
    h, w = prev.shape[:2]
    setting = (estimator, radius, "compensated", capi.SEMANTICS_INTENDED)
    mv = chain.vectors(estimator, radius, capi.SEMANTICS_INTENDED)
    want = [ex.extrapolate(prev, curr, mv, a) for a in AHEADS]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    outs = [ctx.create_frame(w, h) for _ in AHEADS]
    try:
        apply(ctx, setting)
        ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
        for fused in (False, True):                                   # the fused order does not apply
            ctx.set_fused_motion_interpolate(fused)
            ctx.interpolate_frames(p, c, outs[0], AHEADS[1])
            got = ctx.download(outs[0])
            assert (got == want[1]).all(), first_bad(got, want[1])
            ctx.interpolate_frames_multi(p, c, outs, AHEADS)
            for a, o, e in zip(AHEADS, outs, want):
                got = ctx.download(o)
                assert (got == e).all(), f"a={a}: {first_bad(got, e)}"
        ctx.set_fused_motion_interpolate(False)
        # static protection has no effect on extrapolated frames
        ctx.set_static_protection(8)
        ctx.interpolate_frames(p, c, outs[0], AHEADS[0])
        assert (ctx.download(outs[0]) == want[0]).all()
        ctx.set_static_protection(-1)
        # an invalid value is refused and the setting stays
        assert ctx.lib.lfg_set_generation(ctx.h, 7) == -1
        ctx.interpolate_frames(p, c, outs[0], AHEADS[0])
        assert (ctx.download(outs[0]) == want[0]).all()
        # INTERPOLATE restored: the compensated interpolation's bytes again
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        ctx.interpolate_frames(p, c, outs[0], 0.5)
        back = chain.frames(setting, [0.5])[0]
        assert (ctx.download(outs[0]) == back).all()
        assert not (back == want[0]).all()
    finally:
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        ctx.set_static_protection(-1)
        apply(ctx, DEFAULT)
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


def test_generation_switch_restores_the_compensated_call(ctx):
    """With INTERPOLATE restored the bytes equal lfg_interpolate_compensated's on the same vectors."""
    prev, curr = cases.small_scene(96, 64, 4)
    h, w = prev.shape[:2]
    p, c, o, ref = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h), ctx.create_frame(w, h)
    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    try:
        apply(ctx, COMPENSATED)
        ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
        ctx.interpolate_frames(p, c, o, 0.5)
        ahead = ctx.download(o)
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        ctx.interpolate_frames(p, c, o, 0.5)
        ctx.motion(p, c, m)
        ctx.interpolate_compensated(p, c, m, ref, 0.5)
        assert (ctx.download(o) == ctx.download(ref)).all()
        ctx.extrapolate_compensated(p, c, m, ref, 0.5)
        assert (ahead == ctx.download(ref)).all() and not (ahead == ctx.download(o)).all()
    finally:
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        apply(ctx, DEFAULT)
        for f in (p, c, o, ref, m):
            ctx.destroy_frame(f)


def test_generation_has_no_effect_on_the_shader(ctx):
    prev, curr = cases.small_scene(96, 64, 5)
    h, w = prev.shape[:2]
    p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
    outs = [ctx.create_frame(w, h) for _ in range(2)]
    noise = synth.make_uncorrelated_pair(w, h, 9)[1]
    try:
        for semantics in (capi.SEMANTICS_REFERENCE, capi.SEMANTICS_INTENDED):
            apply(ctx, ("full", -1, "shader", semantics))
            ctx.interpolate_frames(p, c, o, 0.5)
            ctx.interpolate_frames_multi(p, c, outs, [0.25, 0.75])
            want = [ctx.download(f) for f in [o] + outs]
            ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
            ctx.interpolate_frames(p, c, o, 0.5)
            ctx.interpolate_frames_multi(p, c, outs, [0.25, 0.75])
            for f, e in zip([o] + outs, want):
                assert (ctx.download(f) == e).all(), semantics
            ctx.set_cut_detection(200)                                # nor on the shader's fallback: prev below 0.5
            ctx.upload(c, noise)
            ctx.interpolate_frames_multi(p, c, outs, [0.25, 0.75])
            assert (ctx.download(outs[0]) == prev).all() and (ctx.download(outs[1]) == noise).all()
            ctx.set_generation(capi.GENERATION_INTERPOLATE)
            ctx.set_cut_detection(-1)
            ctx.upload(c, curr)
    finally:
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        apply(ctx, DEFAULT)
        for f in [p, c, o] + outs:
            ctx.destroy_frame(f)


def test_a_cut_repeats_the_newest_frame(ctx):
    w, h = 96, 64
    prev, curr = synth.make_uncorrelated_pair(w, h, 3)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    aheads = [0.25, 0.5, 1.0]                                        # 0.25 would give prev under the interpolating fallback
    outs = [ctx.create_frame(w, h) for _ in aheads]
    try:
        apply(ctx, COMPENSATED, threshold=200)
        ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
        ctx.interpolate_frames_multi(p, c, outs, aheads)
        for o in outs:
            assert (ctx.download(o) == curr).all()
        assert ctx.last_pair_stats()[1]
        ctx.interpolate_frames(p, c, outs[0], 0.25)
        assert (ctx.download(outs[0]) == curr).all()
        # no cut: a correlated pair is extrapolated as without detection
        moved = synth.translate(prev, (3, -2))
        ctx.upload(c, moved)
        ctx.interpolate_frames(p, c, outs[0], 0.5)
        assert not ctx.last_pair_stats()[1]
        got = ctx.download(outs[0])
        ctx.set_cut_detection(-1)
        ctx.interpolate_frames(p, c, outs[1], 0.5)
        assert (got == ctx.download(outs[1])).all()
    finally:
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        apply(ctx, DEFAULT)
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (96, 64), (200, 120), (130, 90), (96, 64), (300, 170)]
    inputs = [cases.field("random" if i % 2 else "piecewise", w, h, 60 + i) for i, (w, h) in enumerate(sizes)]
    alone = [run(ctx, a, b, v, 0.75, 1020) for a, b, v in inputs]

    def enqueue(i, a, b, v):
        h, w = a.shape[:2]
        p, c, m = ctx.frame_from(a), ctx.frame_from(b), ctx.frame_from(v, capi.FORMAT_MV_S8X2)
        o = ctx.create_frame(w, h)
        ctx.extrapolate_compensated(p, c, m, o, 0.75, 1020)
        return p, c, m, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- lfg_host --generation

def test_host_presents_the_real_frame_first(tmp_path):
    w, h, n = 64, 36, 4
    aheads = [0.5, 1.0]
    frames = [synth.make_prev(w, h)]
    for k in range(1, n):
        frames.append(synth.translate(frames[-1], (3, -2), synth.BASE_SEED + k))
    options = ("--semantics", "intended", "--interpolator", "compensated", "--factors", "0.5,1.0")
    info, got = host_run(tmp_path / "ahead", frames, (2 * w, 2 * h), "--generation", "extrapolate", *options)
    assert info["presented"] == len(got) == n + 2 * (n - 1) and info["interpolated"] == 2 * (n - 1)
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ups = [c.create_frame(2 * w, 2 * h) for _ in frames]
        for f, u in zip(frames, ups):
            c.scale(c.frame_from(f), u)
        m = c.create_frame(2 * w, 2 * h, capi.FORMAT_MV_S8X2)
        o = c.create_frame(2 * w, 2 * h)
        want = [c.download(ups[0])]
        for k in range(1, n):                                         # real k, then generated k + a1, k + a2
            want.append(c.download(ups[k]))
            c.motion(ups[k - 1], ups[k], m)
            for a in aheads:
                c.extrapolate_compensated(ups[k - 1], ups[k], m, o, a, 48)
                want.append(c.download(o))
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k
    assert not (got[2] == got[1]).all()                               # the generated frames are no copies of the real one
    # --generation interpolate is the run without the option
    _, plain = host_run(tmp_path / "plain", frames, (2 * w, 2 * h), *options)
    _, named = host_run(tmp_path / "named", frames, (2 * w, 2 * h), "--generation", "interpolate", *options)
    assert plain.shape == named.shape == got.shape and (plain == named).all()
    assert (plain[-1] == want[-3]).all()                              # interpolating, the newest real frame comes last


def test_host_evaluate_extrapolating(ctx, tmp_path):
    w, h, n = 96, 64, 5
    frames = [synth.make_prev(w, h, synth.BASE_SEED)]
    for _ in range(n - 1):
        frames.append(synth.translate(frames[-1], (3, -2), synth.BASE_SEED))
    tmp_path.mkdir(exist_ok=True)
    src = tmp_path / "in.rgba"
    np.concatenate([f.reshape(-1) for f in frames]).tofile(src)
    p = subprocess.run([HOST, "--input-width", str(w), "--input-height", str(h), "--frames", str(n), "--quiet", "--input-raw", str(src),
                        "--evaluate", "--semantics", "intended", "--interpolator", "compensated", "--generation", "extrapolate"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    report = json.loads(p.stdout.strip().splitlines()[-1])
    ev = report["evaluation"]
    assert report["presented"] == 0 and ev["pairs"] == 2 and set(ev) == {"pairs", "generated", "repeated"}
    fs = [ctx.frame_from(f) for f in frames]
    o, generated, repeated = ctx.create_frame(w, h), ctx.create_diff_record(), ctx.create_diff_record()
    try:
        apply(ctx, COMPENSATED)
        ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
        for k in range(2):
            ctx.interpolate_frames(fs[2 * k], fs[2 * k + 1], o, 1.0)
            ctx.frame_diff(o, fs[2 * k + 2], generated, accumulate=k > 0)
            ctx.frame_diff(fs[2 * k + 1], fs[2 * k + 2], repeated, accumulate=k > 0)
        for name, record in (("generated", generated), ("repeated", repeated)):
            rec = ctx.read_diff_record(record)
            want = capi.summarize(rec)
            assert [ev[name][k] for k in INT_KEYS] == [want[k] for k in INT_KEYS], (name, ev[name], want)
            assert tuple(ev[name]["sse"]) == rec[1], name
        assert ev["generated"]["differing"] < ev["repeated"]["differing"]
        assert ev["repeated"]["differing"] > w * h                   # frames 2k + 1 and 2k + 2 differ nearly everywhere
    finally:
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        apply(ctx, DEFAULT)
        for f in fs + [o, generated, repeated]:
            ctx.destroy_frame(f)
