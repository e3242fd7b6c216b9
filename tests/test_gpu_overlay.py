"""Static-overlay protection on the GPU, every result byte for byte: lfg_static_mask against numpy, both load paths and any
mask pitch; lfg_interpolate_compensated_masked[_multi] against the CPU model (tests/overlay_model.py) on the overlay scenes,
random fields and the hand-made cases of tests/overlay_cases.py; lfg_set_static_protection in lfg_interpolate_frames[_multi]
against the CPU chain; argument checks; lanes; and the host's --protect-static."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import mc_model as mc
from tests import overlay_cases as oc
from tests import overlay_model as ov
from tests.gpu_kit import apply, ctx, first_bad, gpu_vectors, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

# 1 .. 3 columns alone, a width below and above one wave's 256 pixels, no multiple of 4, more than one block in both directions
SHAPES = [(1, 1), (3, 1), (5, 3), (63, 5), (65, 9), (257, 131), (260, 4)]
FACTORS = cases.DYADIC_FACTORS + cases.INEXACT_FACTORS + cases.LIMIT_FACTORS
FOUR_FACTORS = [0.25, 0.3, 5.0 / 6.0, cases.LIMIT_FACTORS[0]]         # from each of the three lists
POISON = 0x5A


# ---- lfg_static_mask

def pair_with_every_difference(w, h, seed):
    """(prev, curr): half of the pixels equal, the others off by a few levels or by anything."""
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    small = np.clip(prev.astype(np.int16) + rng.integers(-20, 21, prev.shape), 0, 255).astype(np.uint8)
    r = rng.random((h, w))[..., None]
    curr = np.where(r < 0.5, prev, np.where(r < 0.9, small, rng.integers(0, 256, prev.shape, dtype=np.uint8))).astype(np.uint8)
    return prev, curr


@pytest.mark.parametrize("w,h", SHAPES)
def test_static_mask_equals_numpy(ctx, w, h):
    prev, curr = pair_with_every_difference(w, h, 100 * w + h)
    # a row pitch of 16 n bytes takes the 16-byte loads (the base is the allocation's), one of 16 n + 4 the dword loads
    pads = {"16-byte": (-w) % 4 + 4, "dword": (1 - w) % 4 + 4}
    # the mask's rows: tight from the allocation's base, an odd pitch from the base, an odd pitch 1 byte into the allocation
    layouts = [(None, 0), (w + 3 + (w % 2), 0), (w + 3 + (w % 2), 1)]
    for path, pad in pads.items():
        assert ((w + pad) * 4) % 16 == (0 if path == "16-byte" else 4)
        bp, p = pitched(ctx, prev, pad)
        bc, c = pitched(ctx, curr, pad)
        try:
            for tolerance in (0, 47, 1020):
                want = ov.static_mask(prev, curr, tolerance)
                for pitch, offset in layouts:
                    owner, mask = ctx.create_mask(w, h, pitch, offset, POISON)
                    ctx.static_mask(p, c, mask, tolerance)
                    rows, raw = ctx.download_mask(owner, mask)
                    ctx.destroy_frame(owner)
                    assert (rows[:, :w] == want).all(), (path, tolerance, pitch, offset, np.argwhere(rows[:, :w] != want)[:3].tolist())
                    assert (rows[:-1, w:] == POISON).all()                          # the row padding
                    assert (raw[:offset] == POISON).all() and (raw[offset + mask.pitch * (h - 1) + w:] == POISON).all()
        finally:
            ctx.destroy_frame(bp)
            ctx.destroy_frame(bc)
    assert set(np.unique(ov.static_mask(prev, curr, 47))) <= {0, 255}


def test_static_mask_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 40, 24
    prev, curr = pair_with_every_difference(w, h, 1)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    m = ctx.frame_from(np.zeros((h, w, 2), np.int8), capi.FORMAT_MV_S8X2)
    small = ctx.create_frame(w - 1, h)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)
    owner, mask = ctx.create_mask(w, h, w + 8, 0, POISON)

    def call(a, b, out, tolerance=0):
        return lib.lfg_static_mask(ctx.h, a and B(a), b and B(b), tolerance, out and B(out))

    bad = [
        call(None, c, mask), call(p, None, mask), call(p, c, None),
        call(p, c, capi.Mask(None, w, h, w)),
        call(p, c, capi.Mask(mask.data, w - 1, h, w)), call(p, c, capi.Mask(mask.data, w, h + 1, w)),
        call(p, c, capi.Mask(mask.data, w, h, w - 1)),                # pitch < width
        call(p, c, mask, -1), call(p, c, mask, 1021),
        call(p, m, mask), call(capi.Frame(), c, mask), call(small, c, mask), call(odd, c, mask),
        call(p, c, capi.Mask(p.data + 16, w, h, w)), call(p, c, capi.Mask(c.data, w, h, w)),      # the mask overlaps a frame
        lib.lfg_static_mask(None, B(p), B(c), 0, B(mask)),
    ]
    assert all(rc == -1 for rc in bad), bad
    assert lib.lfg_set_static_protection(ctx.h, -2) == -1 and lib.lfg_set_static_protection(ctx.h, 1021) == -1
    assert lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert (ctx.download_mask(owner, mask)[1] == POISON).all()
    assert (ctx.download(p) == prev).all() and (ctx.download(c) == curr).all()
    for f in (p, c, m, small, wide, owner):
        ctx.destroy_frame(f)


# ---- lfg_interpolate_compensated_masked[_multi]

def run_masked(ctx, prev, curr, mv, mask, factors, match_sad, multi=False, pads=None):
    """The frames of the masked call, one per factor; with pads = (prev, curr, mv, out, mask) every array sits in wider rows."""
    h, w = prev.shape[:2]
    pp, pc, pm, po, pk = pads or (0, 0, 0, 0, 0)
    owners = []

    def frame(host, pad, fmt=capi.FORMAT_RGBA8):
        if pad == 0:
            owners.append(ctx.frame_from(host, fmt))
            return owners[-1]
        big, view = pitched(ctx, host, pad, fmt)
        owners.append(big)
        return view

    p, c, m = frame(prev, pp), frame(curr, pc), frame(mv, pm, capi.FORMAT_MV_S8X2)
    outs = [frame(np.zeros((h, w, 4), np.uint8), po) for _ in (factors if multi else factors[:1])]
    out_owners = owners[3:]
    owner, k = ctx.mask_from(mask, w + pk if pk else None, 1 if pk else 0, POISON)
    owners.append(owner)
    try:
        got = []
        if multi:
            ctx.interpolate_compensated_masked_multi(p, c, m, k, outs, factors, match_sad)
            raws = [ctx.download(o) for o in out_owners]
        else:
            raws = []
            for t in factors:
                ctx.interpolate_compensated_masked(p, c, m, k, outs[0], t, match_sad)
                raws.append(ctx.download(out_owners[0]))
        for raw in raws:
            assert (raw[:, w:] == POISON).all()                         # the outputs' padding is not written
            got.append(raw[:, :w])
        assert (ctx.download_mask(owner, k)[0][:, :w] == mask).all()    # the mask is only read
        return got
    finally:
        for f in owners:
            ctx.destroy_frame(f)


def check_against_model(ctx, prev, curr, mv, mask, factors, match_sad, what, **how):
    got = run_masked(ctx, prev, curr, mv, mask, factors, match_sad, **how)
    for t, g in zip(factors, got):
        want = ov.interpolate_masked(prev, curr, mv, mask, t, match_sad)
        assert (g == want).all(), f"{what} t={t} {how}: {first_bad(g, want)}"
    return got


@pytest.mark.parametrize("w,h", SHAPES + [(200, 120)])
def test_masked_random_field_equals_the_model(ctx, w, h):
    prev, curr, mv, mask, ms = oc.random_masked(w, h, 7 * w + h)
    single = check_against_model(ctx, prev, curr, mv, mask, FOUR_FACTORS, ms, "random")
    multi = check_against_model(ctx, prev, curr, mv, mask, FOUR_FACTORS, ms, "random", multi=True)
    padded = check_against_model(ctx, prev, curr, mv, mask, FOUR_FACTORS, ms, "random", multi=True, pads=(3, 5, 7, 9, 11))
    assert all((a == b).all() and (a == c).all() for a, b, c in zip(single, multi, padded))
    # an all-zero mask: lfg_interpolate_compensated's bytes, from the GPU
    zero = np.zeros((h, w), np.uint8)
    got = run_masked(ctx, prev, curr, mv, zero, FOUR_FACTORS, ms)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o = ctx.create_frame(w, h)
    try:
        for t, g in zip(FOUR_FACTORS, got):
            ctx.interpolate_compensated(p, c, m, o, t, ms)
            assert (g == ctx.download(o)).all(), t
    finally:
        for f in (p, c, m, o):
            ctx.destroy_frame(f)


@pytest.mark.parametrize("kind,pan", oc.SCENES)
def test_masked_overlay_scenes_equal_the_model(ctx, kind, pan):
    prev, curr, truth, on = oc.scene(kind, pan)
    mv = gpu_vectors(ctx, prev, curr, "full")
    mask = ov.static_mask(prev, curr, 0)
    assert mask[on].all()
    got = check_against_model(ctx, prev, curr, mv, mask, [0.5, 0.3], 48, f"{kind} {pan}")[0]
    assert not (oc.wrong(got, truth) & on).any()                        # the overlay itself is exact


def test_masked_hand_made_cases(ctx):
    """Each case at every factor equals the model; at t = 0.5 the literal values of test_overlay_model.py."""
    outs = {name: check_against_model(ctx, *case[:4], FACTORS, case[4], name)[FACTORS.index(0.5)]
            for name, case in oc.hand_made().items()}
    prev, curr = oc.static_under_collision()[:2]
    assert (outs["static under collision"][4, 5] == prev[4, 6]).all()
    assert (outs["mask byte 1"] == outs["static under collision"]).all() and (outs["mask byte 128"] == outs["mask byte 1"]).all()
    prev = oc.walk_past_static_run()[0]
    assert (outs["walk past a static run"][0, 5] == prev[0, 3]).all()
    prev, curr = oc.rule_on_projected_pixels()[:2]
    assert (outs["rule on projected pixels"][2, 6] == curr[2, 5]).all() and (outs["rule on projected pixels"][5, 6] == prev[5, 7]).all()
    assert (outs["rule on a hole, p static"][0, 8] == oc.rule_on_a_hole(True)[1][0, 9]).all()
    assert (outs["rule on a hole, c static"][0, 8] == oc.rule_on_a_hole(False)[0][0, 6]).all()


def test_masked_walk_reaches_16(ctx):
    """cases.mc_walk_reach through the masked call, byte for byte the model: under an all-zero mask the holes at distance 16
    are filled from the one projected pixel and those at 17 are not; with (26 .. 29, 20) static the walk passes over the run
    and (36, 20) is still filled."""
    prev, curr, mv, blank = cases.mc_walk_reach()
    factors, ms = list(cases.WALK_REACH_FACTORS), cases.WALK_REACH_MATCH_SAD
    for mask, static_run in ((np.zeros((40, 40), np.uint8), False), (cases.walk_reach_static_run(), True)):
        got = check_against_model(ctx, prev, curr, mv, mask, factors, ms, f"walk reach, run {static_run}")
        got_blank = check_against_model(ctx, prev, curr, blank, mask, factors, ms, f"walk reach, blank, run {static_run}")
        for t, g, b in zip(factors, got, got_blank):
            cases.check_walk_reach(g, b, (t, static_run), static_run=static_run)


def test_masked_region_of_interest(ctx):
    prev, curr, mv, mask, ms, (x, y, w, h) = oc.region_of_interest()
    H, W = prev.shape[:2]
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    o = ctx.frame_from(np.full((H, W, 4), POISON, np.uint8))
    owner, k = ctx.mask_from(mask)
    try:
        view = lambda f, bpp, fmt: capi.Context.wrap(f.data + y * f.pitch + x * bpp, w, h, fmt, pitch=f.pitch)
        roi_mask = capi.Mask(k.data + y * k.pitch + x, w, h, k.pitch)
        ctx.interpolate_compensated_masked(view(p, 4, capi.FORMAT_RGBA8), view(c, 4, capi.FORMAT_RGBA8), view(m, 2, capi.FORMAT_MV_S8X2),
                                           roi_mask, view(o, 4, capi.FORMAT_RGBA8), 0.3, ms)
        raw = ctx.download(o)
        want = ov.interpolate_masked(*(a[y:y + h, x:x + w] for a in (prev, curr, mv, mask)), 0.3, ms)
        assert (raw[y:y + h, x:x + w] == want).all(), first_bad(raw[y:y + h, x:x + w], want)
        raw[y:y + h, x:x + w] = POISON
        assert (raw == POISON).all()                                    # nothing outside the ROI is written
    finally:
        for f in (p, c, m, o, owner):
            ctx.destroy_frame(f)


def test_masked_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 40, 24
    prev, curr, mv, mask, ms = oc.random_masked(w, h, 5)
    p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
    pattern = np.full((h, w, 4), POISON, np.uint8)
    o, o2 = ctx.frame_from(pattern), ctx.frame_from(pattern)
    owner, k = ctx.mask_from(mask)

    def single(mk, out=o, t=0.5, match=48, a=p):
        return lib.lfg_interpolate_compensated_masked(ctx.h, a and B(a), B(c), B(m), mk and B(mk), out and B(out), t, match)

    def multi(mk, outs, factors, match=48):
        po = (capi._FP * len(outs))(*[ctypes.pointer(f) for f in outs])
        pf = (ctypes.c_float * len(factors))(*factors)
        return lib.lfg_interpolate_compensated_masked_multi(ctx.h, B(p), B(c), B(m), mk and B(mk), po, pf, len(outs), match)

    bad = [
        single(None), single(capi.Mask(None, w, h, w)),
        single(capi.Mask(k.data, w - 1, h, w)), single(capi.Mask(k.data, w, h - 1, w)), single(capi.Mask(k.data, w, h, w - 1)),
        single(capi.Mask(o.data, w, h, w)),                           # the mask overlaps the output
        single(k, None), single(k, o, float("nan")), single(k, o, 1.01), single(k, o, 0.5, 1021), single(k, o, 0.5, 48, None),
        single(k, p),                                                 # the compensated call's own rules
        multi(None, [o, o2], [0.25, 0.5]), multi(k, [o, o], [0.25, 0.5]), multi(k, [o, o2], [0.25, float("inf")]),
        multi(capi.Mask(o2.data, w, h, w), [o, o2], [0.25, 0.5]),
    ]
    assert all(rc == -1 for rc in bad), bad
    ctx.sync()
    assert (ctx.download(o) == pattern).all() and (ctx.download(o2) == pattern).all()
    for f in (p, c, m, o, o2, owner):
        ctx.destroy_frame(f)


def test_masked_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (65, 9), (200, 120), (130, 90), (5, 3), (257, 131)]
    inputs = [oc.random_masked(w, h, 40 + i)[:4] for i, (w, h) in enumerate(sizes)]
    alone = [run_masked(ctx, *a, [0.3], 1020)[0] for a in inputs]
    masks = []

    def enqueue(i, prev, curr, mv, mask):
        h, w = prev.shape[:2]
        p, c, m = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)
        owner, k = ctx.mask_from(mask)
        masks.append(k)                                               # (the struct must outlive the call only; kept for the frames' sake)
        o = ctx.create_frame(w, h)
        ctx.interpolate_compensated_masked(p, c, m, k, o, 0.3, 1020)
        return p, c, m, owner, o

    three_lanes(ctx, inputs, enqueue, alone)


# ---- lfg_set_static_protection in lfg_interpolate_frames[_multi]

_chains = {}


def chain_of(prev, curr):
    key = (prev.tobytes(), curr.tobytes())
    if key not in _chains:
        _chains[key] = cases.Chain(prev, curr)
    return _chains[key]


def expected(prev, curr, setting, tolerance, factors, match_sad=48):
    """The CPU chain: the estimator's model, the refine model, then the compensated model, or with a tolerance the numpy mask
    and the overlay model."""
    chain = chain_of(prev, curr)
    if tolerance < 0 or setting[2] != "compensated":
        return chain.frames(setting, factors, match_sad)
    mv = chain.vectors(setting[0], setting[1], setting[3])
    mask = ov.static_mask(prev, curr, tolerance)
    return [ov.interpolate_masked(prev, curr, mv, mask, t, match_sad) for t in factors]


def glyph_pair():
    return oc.scene("glyphs", (6, -4))[:2]


@pytest.fixture
def settings_restored(ctx):
    yield
    ctx.set_static_protection(-1)
    apply(ctx, ("full", -1, "shader", capi.SEMANTICS_REFERENCE))


@pytest.mark.parametrize("estimator", cases.ESTIMATORS)
@pytest.mark.parametrize("radius", [-1, 1])
def test_dispatch_equals_the_chain(ctx, settings_restored, estimator, radius):
    prev, curr = glyph_pair()
    h, w = prev.shape[:2]
    setting = (estimator, radius, "compensated", capi.SEMANTICS_INTENDED)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    outs = [ctx.create_frame(w, h) for _ in cases.MATRIX_FACTORS]
    try:
        apply(ctx, setting)
        ctx.set_static_protection(0)
        ctx.interpolate_frames(p, c, outs[0], cases.MATRIX_FACTOR)
        want = expected(prev, curr, setting, 0, [cases.MATRIX_FACTOR])[0]
        got = ctx.download(outs[0])
        assert (got == want).all(), first_bad(got, want)
        assert (got != chain_of(prev, curr).frames(setting, [cases.MATRIX_FACTOR])[0]).any()      # the setting shows on this pair
        ctx.interpolate_frames_multi(p, c, outs, cases.MATRIX_FACTORS)
        for t, o, want in zip(cases.MATRIX_FACTORS, outs, expected(prev, curr, setting, 0, cases.MATRIX_FACTORS)):
            got = ctx.download(o)
            assert (got == want).all(), (t, first_bad(got, want))
        # cut detection around it: a threshold of 0 never cuts
        apply(ctx, setting, threshold=0)
        ctx.interpolate_frames(p, c, outs[1], cases.MATRIX_FACTOR)
        assert (ctx.download(outs[1]) == expected(prev, curr, setting, 0, [cases.MATRIX_FACTOR])[0]).all()
    finally:
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


SETTING = ("full", -1, "compensated", capi.SEMANTICS_INTENDED)


def test_setting_changes_between_enqueued_calls(ctx, settings_restored):
    prev, curr = glyph_pair()
    h, w = prev.shape[:2]
    tolerances = (-1, 0, 24, -1)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    outs = [ctx.create_frame(w, h) for _ in tolerances]
    try:
        apply(ctx, SETTING)
        for tolerance, o in zip(tolerances, outs):
            ctx.set_static_protection(tolerance)
            ctx.interpolate_frames(p, c, o, 0.5)
        ctx.sync()                                                     # the one sync
        for tolerance, o in zip(tolerances, outs):
            want = expected(prev, curr, SETTING, tolerance, [0.5])[0]
            got = ctx.download(o)
            assert (got == want).all(), (tolerance, first_bad(got, want))
    finally:
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


TEMPORARY_SIZES = [(200, 120), (64, 40), (200, 120), (37, 23), (1, 1)]     # large, small, large, odd, 1 x 1


def temporary_pairs():
    return [glyph_pair() if (w, h) == (200, 120) else cases.small_scene(w, h, 9) for w, h in TEMPORARY_SIZES]


def test_mask_temporary_follows_the_size(ctx, settings_restored):
    apply(ctx, SETTING)
    ctx.set_static_protection(0)
    frames = []
    for prev, curr in temporary_pairs():
        h, w = prev.shape[:2]
        p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
        ctx.interpolate_frames(p, c, o, 0.5)
        frames.append((p, c, o))
    ctx.sync()
    for (prev, curr), (p, c, o) in zip(temporary_pairs(), frames):
        want = expected(prev, curr, SETTING, 0, [0.5])[0]
        got = ctx.download(o)
        assert (got == want).all(), (prev.shape, first_bad(got, want))
        for f in (p, c, o):
            ctx.destroy_frame(f)


def test_dispatch_on_three_lanes(ctx, settings_restored):
    apply(ctx, SETTING)
    ctx.set_static_protection(0)
    pairs = temporary_pairs()
    alone = [expected(prev, curr, SETTING, 0, [0.5])[0] for prev, curr in pairs]

    def enqueue(i, prev, curr):
        h, w = prev.shape[:2]
        p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
        ctx.interpolate_frames(p, c, o, 0.5)
        return p, c, o

    three_lanes(ctx, pairs, enqueue, alone)


def test_shader_interpolator_ignores_the_setting(ctx, settings_restored):
    prev, curr = glyph_pair()
    h, w = prev.shape[:2]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    outs = [ctx.create_frame(w, h) for _ in range(2)]
    try:
        for semantics in cases.SEMANTICS:
            apply(ctx, ("full", -1, "shader", semantics))
            ctx.set_static_protection(-1)
            ctx.interpolate_frames(p, c, outs[0], 0.5)
            ctx.set_static_protection(0)
            ctx.interpolate_frames(p, c, outs[1], 0.5)
            assert (ctx.download(outs[0]) == ctx.download(outs[1])).all(), semantics
    finally:
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


def test_a_context_returned_to_off_is_a_context_that_never_left(ctx, settings_restored):
    prev, curr = glyph_pair()
    h, w = prev.shape[:2]

    def frames_of(c, visit):
        p, q = c.frame_from(prev), c.frame_from(curr)
        outs = [c.create_frame(w, h) for _ in cases.MATRIX_FACTORS]
        apply(c, SETTING)
        if visit:
            c.set_static_protection(24)
            c.interpolate_frames(p, q, outs[0], 0.5)
            c.set_static_protection(-1)
        c.interpolate_frames_multi(p, q, outs, cases.MATRIX_FACTORS)
        got = [c.download(o) for o in outs]
        for f in [p, q] + outs:
            c.destroy_frame(f)
        return got

    with capi.Context(0) as fresh:
        never = frames_of(fresh, False)
    back = frames_of(ctx, True)
    assert all((a == b).all() for a, b in zip(never, back))
    assert all((a == b).all() for a, b in zip(never, expected(prev, curr, SETTING, -1, cases.MATRIX_FACTORS)))


# ---- the host

def test_host_protect_static_matches_the_chain(tmp_path):
    """lfg_host --interpolator compensated --protect-static 0 on a glyph stream: every generated frame is the CPU chain's on the
    frames the host interpolates between (its own 1:1 upscale of the input)."""
    n, pan = 3, (6, -4)
    bg = synth.make_prev(oc.W, oc.H, oc.SEED)
    on, px = oc.overlay("glyphs")
    frames = []
    for k in range(n):
        f = synth.translate(bg, (k * pan[0], k * pan[1]), oc.SEED) if k else bg.copy()
        f[on] = px[on]
        frames.append(f)
    info, got = host_run(tmp_path, frames, (oc.W, oc.H), "--semantics", "intended", "--interpolator", "compensated", "--protect-static", "0")
    assert len(got) == 2 * n - 1
    assert info["protect_static"] == 0
    with capi.Context(0) as c:
        ups = []
        for f in frames:
            i, u = c.frame_from(f), c.create_frame(oc.W, oc.H)
            c.scale(i, u)
            ups.append(c.download(u))
    for k in range(1, n):
        assert (got[2 * k] == ups[k]).all(), k
        want = expected(ups[k - 1], ups[k], SETTING, 0, [0.5])[0]
        assert (got[2 * k - 1] == want).all(), (k, first_bad(got[2 * k - 1], want))
        assert not (oc.wrong(got[2 * k - 1], ups[k]) & on).any()           # the glyphs stand still
