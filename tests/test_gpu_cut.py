"""Scene-cut detection on the GPU: lfg_pair_match against the CPU model (tests/pair_model.py) in exact integers, lfg_cut_fallback
on hand-written records, both behind lfg_interpolate_frames[_multi] against the CPU chain (tests/cases.py), the switch back
to off, three lanes, argument checks, and the host's --cut-threshold.  The threshold of 500 rests on
tests/test_pair_model.py: moving content matches on 700 pixels per thousand or more, cuts on 50 or fewer."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import pair_model as pair
from tests.gpu_kit import DEFAULT, apply, ctx, first_bad, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

MATCH_SADS = [0, 48, 1020]
SEAM_SIZES = [(1, 1), (3, 2), (63, 5), (64, 4), (65, 9), (200, 120), (257, 131)]     # the wave, row and workgroup seams
THRESHOLD = 500
POISON = 0xA5
BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0.0)))
FALLBACK_FACTORS = [0.0, 0.3, BELOW_HALF, 0.5, 0.9, 1.0]                              # prev, prev, prev, curr, curr, curr


def graded_case(w, h, seed):
    """(prev, curr, mv): dense random vectors over the whole byte range (cases.field), and a curr that the gate grades: a
    quarter of the pixels are prev(q + v) exactly (0 outside the image), a quarter that within +-3 per channel, a quarter
    within +-14 (SADs on both sides of 48), a quarter unrelated."""
    prev, noise, mv = cases.field("random", w, h, seed)
    rng = np.random.default_rng(seed + 1000)
    grade = rng.integers(0, 4, (h, w))
    amp = np.array([0, 3, 14, 0])[grade][..., None]
    near = np.clip(cases.warp(prev, mv).astype(np.int16) + np.clip(rng.integers(-14, 15, prev.shape), -amp, amp), 0, 255).astype(np.uint8)
    return prev, np.where((grade == 3)[..., None], noise, near), mv


def poisoned_record(ctx):
    r = ctx.create_pair_record()
    ctx.upload(r, np.full((1, 6, 4), 0xFF, np.uint8))
    return r


# ---- 1. lfg_pair_match equals the model exactly

def check_pair_match(ctx, prev, curr, mv, frames, what):
    p, c, m = frames
    r = poisoned_record(ctx)
    try:
        for sad in MATCH_SADS:
            want = pair.pair_stats(prev, curr, mv, sad)
            ctx.pair_match(p, c, m, r, sad)
            first = ctx.read_pair_record(r)
            ctx.pair_match(p, c, m, r, sad)                   # into the same record: it writes, it does not accumulate
            again = ctx.read_pair_record(r)
            assert first == want and again == want, f"{what} match_sad={sad}: {first} then {again}, model {want}"
    finally:
        ctx.destroy_frame(r)


@pytest.mark.parametrize("w,h", SEAM_SIZES + [(1920, 1080)])
def test_pair_match_equals_the_model(ctx, w, h):
    prev, curr, mv = graded_case(w, h, 31 * w + h)
    if w * h >= 1000:                                         # the gate decides something at every threshold
        counts = [pair.pair_stats(prev, curr, mv, s)[1] for s in MATCH_SADS]
        assert 0 < counts[0] < counts[1] < counts[2] == w * h, counts
    frames = [ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)]
    try:
        check_pair_match(ctx, prev, curr, mv, frames, f"{w}x{h}")
    finally:
        for f in frames:
            ctx.destroy_frame(f)


@pytest.mark.parametrize("w,h", SEAM_SIZES)
def test_pair_match_pitched(ctx, w, h):
    prev, curr, mv = graded_case(w, h, 17 * w + h)
    bp, p = pitched(ctx, prev, 3)
    bc, c = pitched(ctx, curr, 5)
    bm, m = pitched(ctx, mv, 7, capi.FORMAT_MV_S8X2)
    try:
        check_pair_match(ctx, prev, curr, mv, (p, c, m), f"pitched {w}x{h}")
    finally:
        for f in (bp, bc, bm):
            ctx.destroy_frame(f)


# ---- 2. 64-bit sums

def test_sums_beyond_32_bits(ctx):
    w, h = 3840, 2160
    p, c = ctx.create_frame(w, h), ctx.create_frame(w, h)
    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    r = poisoned_record(ctx)
    try:
        ctx.upload(p, np.zeros((h, w, 4), np.uint8))
        ctx.upload(c, np.full((h, w, 4), 255, np.uint8))
        ctx.upload(m, np.zeros((h, w, 2), np.int8))
        ctx.pair_match(p, c, m, r, 1019)
        assert ctx.read_pair_record(r) == (8_294_400, 0, 8_460_288_000)
        ctx.pair_match(p, c, m, r, 1020)
        assert ctx.read_pair_record(r) == (8_294_400, 8_294_400, 8_460_288_000)
    finally:
        for f in (p, c, m, r):
            ctx.destroy_frame(f)


# ---- 3. lfg_cut_fallback alone, on records written by hand

def boundary(pixels, matched):
    """(the largest threshold under which the record is no cut, the smallest under which it is one, or None past 1000)."""
    no_cut = max(t for t in range(1001) if not pair.cut((pixels, matched, 0), t))
    return no_cut, (no_cut + 1 if no_cut < 1000 else None)


@pytest.mark.parametrize("w,h,matched", [(40, 25, 500), (40, 25, 0), (40, 25, 999), (63, 5, 100), (1, 1, 0), (1, 1, 1)])
def test_cut_fallback_on_hand_written_records(ctx, w, h, matched):
    prev, curr = cases.textured(w, h, 90), cases.textured(w, h, 91)
    no_cut, is_cut = boundary(w * h, matched)
    if (w, h) == (40, 25):                                    # 1000 pixels: permille m is no cut, m + 1 is one
        assert (no_cut, is_cut) == (matched, matched + 1)
    if (w, h, matched) == (63, 5, 100):                       # 100 of 315: 317 * 315 = 99,855 <= 100,000 < 100,170 = 318 * 315
        assert (no_cut, is_cut) == (317, 318)
    if (w, h) == (1, 1):
        assert (no_cut, is_cut) == ((0, 1) if matched == 0 else (1000, None))
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    r = ctx.create_pair_record()
    ctx.write_pair_record(r, w * h, matched, 12345)
    poison = np.full((h, w, 4), POISON, np.uint8)
    wide = [pitched(ctx, poison, 2 + i) for i in range(len(FALLBACK_FACTORS))]
    outs = [view for _, view in wide]
    try:
        ctx.cut_fallback(p, c, r, no_cut, outs, FALLBACK_FACTORS)
        for i, (big, _) in enumerate(wide):
            raw = ctx.download(big)
            assert (raw[:, :w] == POISON).all() and (raw[:, w:] == 0x5A).all(), f"no cut at {no_cut}: output {i} was written"
        if is_cut is not None:
            ctx.cut_fallback(p, c, r, is_cut, outs, FALLBACK_FACTORS)
            for i, ((big, _), want) in enumerate(zip(wide, pair.fallback(prev, curr, FALLBACK_FACTORS))):
                raw = ctx.download(big)
                assert (raw[:, :w] == want).all(), f"cut at {is_cut}: output {i}: {first_bad(raw[:, :w], want)}"
                assert (raw[:, :w] == (curr if i >= 3 else prev)).all()
                assert (raw[:, w:] == 0x5A).all(), f"cut at {is_cut}: the padding of output {i} was written"
        assert ctx.read_pair_record(r) == (w * h, matched, 12345)          # the record is read, never written
        assert (ctx.download(p) == prev).all() and (ctx.download(c) == curr).all()
    finally:
        for f in [p, c, r] + [big for big, _ in wide]:
            ctx.destroy_frame(f)


def test_cut_fallback_with_every_output(ctx):
    w, h, n = 63, 5, 16                                       # LFG_MAX_FACTORS
    prev, curr = cases.textured(w, h, 92), cases.textured(w, h, 93)
    factors = [k / (n - 1) for k in range(n)]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    r = ctx.create_pair_record()
    outs = [ctx.frame_from(np.full((h, w, 4), POISON, np.uint8)) for _ in range(n)]
    try:
        ctx.write_pair_record(r, w * h, 157, 0)               # 157,000 < 500 * 315 = 157,500 <= 158,000
        ctx.cut_fallback(p, c, r, THRESHOLD, outs, factors)
        for t, o, want in zip(factors, outs, pair.fallback(prev, curr, factors)):
            assert (ctx.download(o) == want).all(), t
        for o in outs:
            ctx.upload(o, np.full((h, w, 4), POISON, np.uint8))
        ctx.write_pair_record(r, w * h, 158, 0)
        ctx.cut_fallback(p, c, r, THRESHOLD, outs, factors)
        for o in outs:
            assert (ctx.download(o) == POISON).all()
    finally:
        for f in [p, c, r] + outs:
            ctx.destroy_frame(f)


# ---- 4. behind both entry points, held to the CPU chain

SETTINGS = [("full", -1, "shader", 0), ("full", -1, "shader", 1), ("full", 1, "compensated", 1),
            ("pyramid", -1, "compensated", 1), ("pyramid", 2, "compensated", 0), ("pyramid", 0, "shader", 1)]
FACTORS = [cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS         # the single call, then the multi call


def cut_scene(w=200, h=120):
    """Two synth frames of different seeds: the same gradient under unrelated noise."""
    return synth.make_prev(w, h, synth.BASE_SEED), synth.make_prev(w, h, synth.BASE_SEED + 1)


_chains = {}


def chain_of(name):
    if name not in _chains:
        _chains[name] = cases.Chain(*(cases.matrix_scene() if name == "matrix" else cut_scene()))
    return _chains[name]


def both_calls(ctx, p, c, outs, detecting):
    """The single call into outs[0] and the multi call into outs[1:], over poisoned outputs: the frames, and what
    lfg_last_pair_stats says after each call (None with detection off)."""
    h, w = outs[0].height, outs[0].width
    for o in outs:
        ctx.upload(o, np.full((h, w, 4), POISON, np.uint8))
    ctx.interpolate_frames(p, c, outs[0], FACTORS[0])
    single = ctx.last_pair_stats() if detecting else None
    ctx.interpolate_frames_multi(p, c, outs[1:], FACTORS[1:])
    multi = ctx.last_pair_stats() if detecting else None
    return [ctx.download(o) for o in outs], single, multi


@pytest.fixture(scope="module")
def scenes(ctx):
    made = {}
    for name in ("matrix", "cut"):
        ch = chain_of(name)
        h, w = ch.prev.shape[:2]
        made[name] = (ch, ctx.frame_from(ch.prev), ctx.frame_from(ch.curr), [ctx.create_frame(w, h) for _ in FACTORS])
    yield made
    for _, p, c, outs in made.values():
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(str(v) for v in s))
def test_entry_points_equal_the_chain(ctx, scenes, setting, fused):
    try:
        apply(ctx, setting, fused, threshold=THRESHOLD)
        results = {name: both_calls(ctx, p, c, outs, True) for name, (_, p, c, outs) in scenes.items()}
    finally:
        apply(ctx, DEFAULT)
    for name, (got, single, multi) in results.items():
        ch = scenes[name][0]
        stats = pair.pair_stats(ch.prev, ch.curr, ch.vectors(*setting[:2], setting[3]), capi.DEFAULT_MATCH_SAD)
        is_cut = name == "cut"
        assert pair.cut(stats, THRESHOLD) == is_cut, (name, stats)
        assert single == (stats, is_cut) and multi == (stats, is_cut), f"{name} {setting}: {single}, {multi}, model {stats}"
        want = pair.fallback(ch.prev, ch.curr, FACTORS) if is_cut else ch.frames(setting, FACTORS)
        for t, g, e in zip(FACTORS, got, want):
            assert (g == e).all(), f"{name} {setting} fused={fused} t={t}: {first_bad(g, e)}"
    # on the cut: prev for 0.3, then prev, curr, curr, curr for 0.25, 5/6, 0.5, 0.9
    ch = scenes["cut"][0]
    for g, from_curr in zip(results["cut"][0], [False, False, True, True, True]):
        assert (g == (ch.curr if from_curr else ch.prev)).all()


# ---- 5. off means off

def test_off_means_off(ctx, scenes):
    with capi.Context(0) as fresh:
        rc = fresh.lib.lfg_last_pair_stats(fresh.h, None, None)
        assert rc == -1 and fresh.lib.lfg_last_pair_stats(fresh.h, ctypes.byref(capi.PairStats()), None) == -1
        assert fresh.lib.lfg_last_error(fresh.h).decode()
        try:
            ctx.set_cut_detection(THRESHOLD)
            for _, p, c, outs in scenes.values():             # the switch has been used before it goes back
                ctx.interpolate_frames(p, c, outs[0], 0.5)
            ctx.set_cut_detection(-1)
            for name, (ch, p, c, outs) in scenes.items():
                used = both_calls(ctx, p, c, outs, False)[0]
                h, w = ch.prev.shape[:2]
                fp, fc = fresh.frame_from(ch.prev), fresh.frame_from(ch.curr)
                fo = [fresh.create_frame(w, h) for _ in FACTORS]
                never = both_calls(fresh, fp, fc, fo, False)[0]
                for t, u, n, e in zip(FACTORS, used, never, ch.frames(DEFAULT, FACTORS)):
                    assert (u == n).all(), f"{name} t={t}: {first_bad(u, n)}"
                    assert (n == e).all(), f"{name} t={t}: {first_bad(n, e)}"
                if name == "cut":                             # with detection off a cut is interpolated like any pair
                    assert any((u != ch.prev).any() and (u != ch.curr).any() for u in used)
                for f in [fp, fc] + fo:
                    fresh.destroy_frame(f)
            assert fresh.lib.lfg_last_pair_stats(fresh.h, None, None) == -1      # still no detecting call on that context
        finally:
            ctx.set_cut_detection(-1)


# ---- 6. three lanes

LANE_SIZES = [(200, 120), (64, 36), (33, 17), (1, 1), (130, 90), (64, 36), (200, 120), (7, 5), (33, 17)]
LANE_SETTING = ("full", -1, "compensated", 1)


def lane_pair(k, w, h):
    """Even k: a pan with a moving square (no cut); odd k: two unrelated textures (a cut)."""
    return cases.small_scene(w, h, 40 + k) if k % 2 == 0 else (cases.textured(w, h, 300 + k), cases.textured(w, h, 400 + k))


def test_three_lanes(ctx):
    pairs = [lane_pair(k, w, h) for k, (w, h) in enumerate(LANE_SIZES)]
    alone, alone_stats, lane_stats = [], [], []

    def enqueue(i, prev, curr):
        h, w = prev.shape[:2]
        p, c = ctx.frame_from(prev), ctx.frame_from(curr)
        o = ctx.frame_from(np.full((h, w, 4), POISON, np.uint8))
        ctx.interpolate_frames(p, c, o, cases.MATRIX_FACTOR)
        return p, c, o

    def alone_then_lane_stats():
        """three_lanes takes the first of these after its one sync, while the three lanes still exist: the moment to read
        each lane's record."""
        for lane in range(3):
            ctx.lane_select(lane)
            lane_stats.append(ctx.last_pair_stats())
        yield from alone

    try:
        apply(ctx, LANE_SETTING, threshold=THRESHOLD)
        for k, (prev, curr) in enumerate(pairs):
            fs = enqueue(k, prev, curr)
            alone.append(ctx.download(fs[-1]))
            alone_stats.append(ctx.last_pair_stats())
            for f in fs:
                ctx.destroy_frame(f)
        assert [cut for _, cut in alone_stats] == [k % 2 == 1 for k in range(len(pairs))]
        for k, (prev, curr) in enumerate(pairs):
            if k % 2 == 1:
                assert (alone[k] == prev).all()               # 0.3 < 0.5
            else:
                assert (alone[k] != POISON).any() and (alone[k] != prev).any()
        three_lanes(ctx, pairs, enqueue, alone_then_lane_stats())
    finally:
        apply(ctx, DEFAULT)
    assert len(lane_stats) == 3
    for lane, k in enumerate((6, 7, 8)):                      # each lane's last pair
        prev, curr = pairs[k]
        mv = cases.Chain(prev, curr).vectors(LANE_SETTING[0], LANE_SETTING[1], LANE_SETTING[3])
        want = pair.pair_stats(prev, curr, mv, capi.DEFAULT_MATCH_SAD)
        assert lane_stats[lane] == (want, k % 2 == 1) == alone_stats[k], (lane, lane_stats[lane], want)


# ---- 7. validation

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 40, 25
    prev, curr, mv = graded_case(w, h, 7)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    poison = np.full((h, w, 4), POISON, np.uint8)
    o, o2 = ctx.frame_from(poison), ctx.frame_from(poison)
    r = ctx.create_pair_record()
    ctx.write_pair_record(r, w * h, 0, 77)                    # a cut under any threshold above 0
    small, small_mv = ctx.create_frame(w - 1, h), ctx.create_frame(w, h - 1, capi.FORMAT_MV_S8X2)
    wide, wide_mv = ctx.create_frame(w + 1, h), ctx.create_frame(w + 1, h, capi.FORMAT_MV_S8X2)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)
    shifted = capi.Context.wrap(wide.data + 2, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 4)
    odd_mv = capi.Context.wrap(wide_mv.data, w, h, capi.FORMAT_MV_S8X2, pitch=w * 2 + 1)
    shifted_mv = capi.Context.wrap(wide_mv.data + 1, w, h, capi.FORMAT_MV_S8X2, pitch=w * 2 + 2)
    tall = ctx.frame_from(np.full((2 * h, w, 4), POISON, np.uint8))
    upper = capi.Context.wrap(tall.data, w, h + 1, capi.FORMAT_RGBA8)
    lower = capi.Context.wrap(tall.data + h * w * 4, w, h, capi.FORMAT_RGBA8)      # shares a row with `upper`
    upper_h = capi.Context.wrap(tall.data, w, h, capi.FORMAT_RGBA8)
    inside_prev = capi.Context.wrap(p.data, w, h, capi.FORMAT_RGBA8)
    empty = capi.Frame()
    rec = ctypes.c_void_p(r.data)

    def match(a, b, v, sad=48, stats=rec):
        return lib.lfg_pair_match(ctx.h, a and B(a), b and B(b), v and B(v), sad, stats)

    def fall(a, b, outs, factors=(0.3, 0.9), stats=rec, permille=THRESHOLD, count=None):
        po = (ctypes.POINTER(capi.Frame) * max(len(outs), 1))(*[f and ctypes.pointer(f) for f in outs]) if outs is not None else None
        pf = (ctypes.c_float * max(len(factors), 1))(*factors) if factors is not None else None
        return lib.lfg_cut_fallback(ctx.h, a and B(a), b and B(b), stats, permille, po, pf, (len(outs) if outs is not None else 2) if count is None else count)

    bad = [
        match(None, c, m), match(p, None, m), match(p, c, None), match(empty, c, m), match(p, c, m, stats=None),
        match(p, c, m, stats=ctypes.c_void_p(r.data + 4)),                                   # not 8-byte aligned
        match(p, c, p), match(m, c, m), match(p, m, m),                                      # wrong formats
        match(small, c, m), match(p, small, m), match(p, c, small_mv),                       # wrong sizes
        match(odd, c, m), match(p, odd, m), match(shifted, c, m), match(p, c, odd_mv), match(p, c, shifted_mv),
        match(p, c, m, -1), match(p, c, m, 1021),
        fall(None, c, [o, o2]), fall(p, None, [o, o2]), fall(empty, c, [o, o2]), fall(p, c, [o, o2], stats=None),
        fall(p, c, [o, o2], stats=ctypes.c_void_p(r.data + 4)),
        fall(p, c, None), fall(p, c, [o, o2], factors=None), fall(p, c, [o, None]), fall(p, c, [o, empty]),
        fall(p, c, [o, o2], count=0), fall(p, c, [o] * 17, factors=[0.5] * 17, count=17),
        fall(p, c, [o, o2], permille=-1), fall(p, c, [o, o2], permille=1001),
        fall(p, m, [o, o2]), fall(p, c, [o, m]),                                             # wrong formats
        fall(p, small, [o, o2]), fall(p, c, [o, small]),                                     # wrong sizes
        fall(odd, c, [o, o2]), fall(p, c, [o, odd]), fall(p, c, [o, shifted]),               # pitch, alignment
        fall(p, c, [o, o]), fall(p, c, [o, p]), fall(p, c, [c, o]), fall(p, c, [o, inside_prev]),
        fall(p, c, [upper, lower]),                                                          # overlap without equal pointers
    ]
    assert all(rc == -1 for rc in bad), bad                          # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    for value in (-2, 1001, 100000):
        assert lib.lfg_set_cut_detection(ctx.h, value) == -1
    assert lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert ctx.read_pair_record(r) == (w * h, 0, 77)
    for f in (o, o2):
        assert (ctx.download(f) == POISON).all()
    assert (ctx.download(tall) == POISON).all()
    assert (ctx.download(p) == prev).all() and (ctx.download(c) == curr).all()
    # the failed setter changed nothing: detection is still off, and the valid calls next to the bad ones work
    ctx.interpolate_frames(p, c, o, 0.5)
    ctx.motion(p, c, m)
    ctx.interpolate(p, c, m, o2, 0.5)
    assert (ctx.download(o) == ctx.download(o2)).all()
    assert fall(p, c, [upper_h, lower]) == 0                         # the two halves of `tall` do not overlap
    assert (ctx.download(tall) == np.concatenate([prev, curr])).all()
    # behind the entry points the fallback's rules are checked before anything is enqueued
    try:
        ctx.set_cut_detection(THRESHOLD)
        ctx.upload(tall, np.full((2 * h, w, 4), POISON, np.uint8))
        po = (ctypes.POINTER(capi.Frame) * 2)(ctypes.pointer(upper), ctypes.pointer(lower))
        pf = (ctypes.c_float * 2)(0.3, 0.9)
        assert lib.lfg_interpolate_frames_multi(ctx.h, B(p), B(c), po, pf, 2) == -1
        assert lib.lfg_interpolate_frames(ctx.h, B(p), B(c), B(inside_prev), 0.5) == -1
        ctx.sync()
        assert (ctx.download(tall) == POISON).all() and (ctx.download(p) == prev).all()
    finally:
        ctx.set_cut_detection(-1)
    for f in (p, c, m, o, o2, r, small, small_mv, wide, wide_mv, tall):
        ctx.destroy_frame(f)


# ---- 8. lfg_host --cut-threshold

def test_host_shows_a_source_frame_across_a_cut(ctx, tmp_path):
    w, h = 96, 64
    a, b = synth.make_prev(w, h, synth.BASE_SEED), synth.make_prev(w, h, synth.BASE_SEED + 1)
    frames = [a, synth.translate(a, (3, -2), synth.BASE_SEED), b, synth.translate(b, (3, -2), synth.BASE_SEED + 1)]
    plain_report, plain = host_run(tmp_path / "plain", frames, (w, h), "--semantics", "intended")
    report, got = host_run(tmp_path / "cut", frames, (w, h), "--semantics", "intended", "--cut-threshold", str(THRESHOLD))
    assert plain_report["cuts"] == 0 and plain_report["presented"] == 7
    assert report["cuts"] == 1 and report["presented"] == 7 and report["interpolated"] == 3
    for k in (0, 2, 4, 6):                                    # the real frames: the scale at equal sizes is the identity
        assert (got[k] == frames[k // 2]).all() and (plain[k] == frames[k // 2]).all(), k
    assert (got[3] == frames[2]).all(), first_bad(got[3], frames[2])       # factor 0.5 gives curr
    assert (got[3] == got[4]).all()
    assert (plain[3] != frames[2]).any() and (plain[3] != frames[1]).any()
    for k in (1, 5):
        assert (got[k] == plain[k]).all(), k
    with capi.Context(0) as c:                                # the run without the option is the library's default path
        c.set_semantics(capi.SEMANTICS_INTENDED)
        fs = [c.frame_from(f) for f in frames]
        o = c.create_frame(w, h)
        for k in (1, 2, 3):
            c.interpolate_frames(fs[k - 1], fs[k], o, 0.5)
            assert (c.download(o) == plain[2 * k - 1]).all(), k
