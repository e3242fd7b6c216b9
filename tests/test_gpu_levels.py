"""Level matching on the GPU, every comparison exact: lfg_frame_histogram against np.bincount, lfg_levels_match and lfg_levels_apply
against tests/levels_model.py, and lfg_set_level_matching around lfg_interpolate_frames[_multi] against the model's wrapper around
the existing chains (tests/cases.py, tests/route_cases.py), on the scenes of tests/levels_cases.py -- under every route, with cut
detection either way, on three lanes, with the switch and the frame size changing between enqueued calls.  What the scenes and
the model are held to: tests/test_levels_model.py."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import levels_cases as lc
from tests import levels_model as lm
from tests import pair_model as pair
from tests import route_cases as rc
from tests.gpu_kit import ctx, first_bad, pitched  # noqa: F401  (ctx is a fixture)
from tests.test_gpu_routes import restore, select

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (67, 9), (257, 33), (64, 48)]


def content(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def views(ctx, host, which):
    """`host` on the device as `which` says: "tight"; "padded" (pitch 32 bytes more than a row, padding poisoned); "in1" / "in3",
    a view 1 or 3 pixels into a wider frame whose rows are 16-byte aligned, so the view's base is 4-byte aligned only.  Returns
    (the frame that owns the memory, the view, the owner's host image, the column the view starts at)."""
    h, w = host.shape[:2]
    if which == "tight":
        f = ctx.frame_from(host)
        return f, f, host.copy(), 0
    at = {"padded": 0, "in1": 1, "in3": 3}[which]
    wide_w = (w + at + 8 + 3) // 4 * 4
    wide = np.full((h, wide_w, 4), 0x5A, np.uint8)
    wide[:, at:at + w] = host
    big = ctx.frame_from(wide)
    return big, capi.Context.wrap(big.data + 4 * at, w, h, capi.FORMAT_RGBA8, pitch=wide_w * 4), wide, at


# ---- lfg_frame_histogram

def check_histogram(ctx, view, host, record=None, accumulate=False, before=None):
    rec = record or ctx.create_histogram_record()
    try:
        ctx.frame_histogram(view, rec, accumulate)
        pixels, hist = ctx.read_histogram_record(rec)
        want = lm.histogram(host, before)
        assert pixels == want[0] and (hist == want[1]).all(), np.argwhere(hist != want[1])[:4].tolist()
        return want
    finally:
        if record is None:
            ctx.destroy_frame(rec)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["tight", "padded", "in1", "in3"])
def test_histogram_sizes_and_views(ctx, size, which):
    host = content(*size, 100 * size[0] + size[1])
    big, view, _, _ = views(ctx, host, which)
    try:
        check_histogram(ctx, view, host)
    finally:
        ctx.destroy_frame(big)


def test_histogram_5x3_at_pitch_32_with_poisoned_padding(ctx):
    host = content(5, 3, 7)
    big, view = pitched(ctx, host, 3)                    # 8 pixels a row: pitch 32
    try:
        assert view.pitch == 32
        check_histogram(ctx, view, host)
    finally:
        ctx.destroy_frame(big)


def flat(w, h):
    return np.full((h, w, 4), (17, 200, 3, 255), np.uint8)


def checkerboard(w, h):
    f = np.empty((h, w, 4), np.uint8)
    odd = (np.add.outer(np.arange(h), np.arange(w)) & 1).astype(bool)
    f[odd], f[~odd] = (10, 20, 30, 255), (200, 210, 220, 0)
    return f


def ramp(w, h):
    x = (np.arange(w) % 256).astype(np.uint8)
    return np.broadcast_to(np.stack([x, 255 - x, x ^ 0x55, (x + 128).astype(np.uint8)], -1), (h, w, 4)).copy()


def half_flat_half_noise(w, h):
    f = content(w, h, 31)
    f[: h // 2] = (90, 90, 90, 255)
    return f


CONTENTS = {"flat512x256": lambda: flat(512, 256), "checkerboard": lambda: checkerboard(130, 67), "ramp": lambda: ramp(512, 9),
            "noise": lambda: content(320, 90, 5), "half_flat_half_noise_1080p": lambda: half_flat_half_noise(1920, 1080)}


@pytest.mark.parametrize("name", list(CONTENTS))
def test_histogram_contents(ctx, name):
    """Flat: 131,072 in one bin -- more than 16 bits, every lane of every wave on one address.  The checkerboard: two addresses.
    The ramp: every lane on a bin of its own.  1080p: many workgroups merging, and the grid's tail."""
    host = CONTENTS[name]()
    f = ctx.frame_from(host)
    try:
        check_histogram(ctx, f, host)
    finally:
        ctx.destroy_frame(f)


def test_histogram_accumulates_over_two_frames(ctx):
    a, b = content(67, 9, 1), flat(257, 33)
    fa, fb, rec = ctx.frame_from(a), ctx.frame_from(b), ctx.create_histogram_record()
    try:
        ctx.write_histogram_record(rec, 5, np.full((4, 256), 3, np.uint64))      # what accumulate = 0 must overwrite
        first = check_histogram(ctx, fa, a, rec)
        second = check_histogram(ctx, fb, b, rec, True, first)
        check_histogram(ctx, fa, a, rec, True, second)
    finally:
        for f in (fa, fb, rec):
            ctx.destroy_frame(f)


# ---- lfg_levels_match

def match_cases():
    pairs = dict(lc.record_pairs())
    for name in lc.FADES:
        prev, curr = lc.faded_pan(64, 48, 5, name)
        pairs[name] = (lm.histogram(prev), lm.histogram(curr))
    return pairs


def assert_map(got, want, what):
    for k in ("pixels", "shift_sum", "active", "reserved"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("forward", "inverse"):
        assert (got[k] == want[k]).all(), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


@pytest.mark.parametrize("name", list(match_cases()))
def test_match_equals_the_model(ctx, name):
    a, b = match_cases()[name]
    ra, rb, m = ctx.create_histogram_record(), ctx.create_histogram_record(), ctx.create_levels_map()
    try:
        ctx.write_histogram_record(ra, *a)
        ctx.write_histogram_record(rb, *b)
        for s in lc.MIN_SHIFTS:
            ctx.upload(m, np.full((1, m.width, 4), 0xA5, np.uint8))              # every byte of the map is written
            ctx.levels_match(ra, rb, m, s)
            assert_map(ctx.read_levels_map(m), lm.match(a, b, s), (name, s))
    finally:
        for f in (ra, rb, m):
            ctx.destroy_frame(f)


def test_match_from_the_histograms_the_device_made(ctx):
    """The three calls chained with no host wait between them."""
    prev, curr = lc.faded_pan(67, 9, 5, "gain230plus10")
    p, c, out = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(67, 9)
    ra, rb, m = ctx.create_histogram_record(), ctx.create_histogram_record(), ctx.create_levels_map()
    try:
        ctx.frame_histogram(p, ra)
        ctx.frame_histogram(c, rb)
        ctx.levels_match(ra, rb, m, lc.THRESHOLD)
        ctx.levels_apply(p, out, m, capi.LEVELS_FORWARD)
        want = lm.pair_map(prev, curr, lc.THRESHOLD)
        assert (ctx.download(out) == lm.apply(prev, want, lm.FORWARD)).all()
        assert_map(ctx.read_levels_map(m), want, "chained")
    finally:
        for f in (p, c, out, ra, rb, m):
            ctx.destroy_frame(f)


# ---- lfg_levels_apply

@pytest.fixture(scope="module")
def maps(ctx):
    """(model, device map) of an active and of an inactive pair."""
    models = {"active": lm.pair_map(*lc.faded_pan(64, 48, 5), 0), "inactive": lm.pair_map(*lc.pan(64, 48, 3), lc.THRESHOLD)}
    assert models["active"]["active"] == 1 and models["inactive"]["active"] == 0
    made = {}
    for name, m in models.items():
        f = ctx.create_levels_map()
        ctx.upload(f, lm.map_bytes(m).reshape(1, -1, 4))
        made[name] = (m, f)
    yield made
    for _, f in made.values():
        ctx.destroy_frame(f)


MODES = [(capi.LEVELS_FORWARD, 0.0)] + [(capi.LEVELS_AT, f) for f in lc.FACTORS]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("which", ["tight", "padded", "in1", "in3"])
def test_apply_both_modes_in_place_and_out_of_place(ctx, maps, size, which):
    """Alpha is random in the input and must come out untouched, like every byte of the padding and of the wider frame."""
    w, h = size
    host = content(w, h, 300 * w + h)
    for name, (model, device_map) in maps.items():
        for mode, factor in MODES:
            want = lm.apply(host, model, mode, factor)
            assert (want[..., 3] == host[..., 3]).all() and (name == "active" or (want == host).all())
            # out of place: into a frame of the same layout, poisoned
            src_big, src, _, _ = views(ctx, host, which)
            dst_big, dst, poison, at = views(ctx, np.full_like(host, 0x3C), which)
            try:
                ctx.levels_apply(src, dst, device_map, mode, factor)
                got = ctx.download(dst_big)
                poison[:, at:at + w] = want
                assert (got == poison).all(), (name, mode, factor, first_bad(got, poison))
                # in place
                ctx.levels_apply(src, src, device_map, mode, factor)
                got = ctx.download(src_big)
                poison[...] = 0x5A
                poison[:, at:at + w] = want
                assert which == "tight" or (got == poison).all(), (name, mode, factor, "in place", first_bad(got, poison))
                assert (got[:, at:at + w] == want).all()
            finally:
                ctx.destroy_frame(src_big)
                ctx.destroy_frame(dst_big)


def test_apply_mixed_layouts_take_the_dword_path(ctx, maps):
    """A 16-byte aligned input into an output that is not, and the other way round."""
    host = content(67, 9, 2)
    model, device_map = maps["active"]
    want = lm.apply(host, model, lm.AT, 0.25)
    for a, b in (("tight", "in1"), ("in3", "padded")):
        src_big, src, _, _ = views(ctx, host, a)
        dst_big, dst, poison, at = views(ctx, np.full_like(host, 0x3C), b)
        try:
            ctx.levels_apply(src, dst, device_map, capi.LEVELS_AT, 0.25)
            poison[:, at:at + 67] = want
            assert (ctx.download(dst_big) == poison).all()
        finally:
            ctx.destroy_frame(src_big)
            ctx.destroy_frame(dst_big)


# ---- the switch

FACTORS = [0.3, 0.25, 0.5, 1.0]                      # the single call's, then the multi call's
BASE = ("pyramid", -1, "compensated", 1)
ROUTES = {
    "shader": rc.route(("full", -1, "shader", 0)),
    "shader_fused": rc.route(("full", -1, "shader", 0), fused=True),      # the one route the fused kernels serve: not with the switch on
    "pyramid": rc.route(BASE),
    "full_search": rc.route(("full", -1, "compensated", 1)),
    "refined_subpel": rc.route(("pyramid", 1, "compensated", 1), subpel=1),
    "bidirectional": rc.route(BASE, bidirectional=1),
    "masked": rc.route(BASE, protect=0),
    "extrapolate": rc.route(BASE, generation="extrapolate"),
    "cut_passes": rc.route(BASE, cut="passes"),
    "cut_fails": rc.route(BASE, cut="fails"),
}
_scenes, _chains = {}, {}


def scene_of(name):
    """(prev, curr, min_shift16, the model's map, what the stages see, the chain on that)."""
    if not _scenes:
        _scenes.update(lc.switch_scenes())
    prev, curr, threshold = _scenes[name]
    m = lm.pair_map(prev, curr, threshold)
    seen = lm.apply(prev, m, lm.FORWARD)
    key = seen.tobytes() + curr.tobytes()
    if key not in _chains:
        chain = rc.RouteChain(seen, curr)
        p = pair.permille(chain.stats(ROUTES["pyramid"]))
        assert p - rc.ROOM >= 1
        chain.passes, chain.fails = p - rc.ROOM, (p + rc.ROOM + 1 if p + rc.ROOM + 1 <= 1000 else None)
        _chains[key] = chain
    return prev, curr, threshold, m, seen, _chains[key]


def expected(name, r, factors):
    """The model's wrapper around the chain of what the stages see."""
    prev, curr, threshold, _, _, chain = scene_of(name)
    ahead = r.interpolator == "compensated" and r.generation == "extrapolate"
    frames, m = lm.wrapper(prev, curr, threshold, lambda p, c: chain.frames(r._replace(cut="off"), factors), factors,
                           at_outputs=not ahead, cut=(lambda p, c: chain.is_cut(r)) if r.cut != "off" else None, newest=ahead)
    return frames, m


def run_route(ctx, name, r, min_shift16, frames):
    """Both entry points under the route: (the frames of FACTORS, lfg_last_level_match after each call)."""
    _, _, _, _, _, chain = scene_of(name)
    p, c, outs = frames
    select(ctx, chain, r)
    ctx.set_level_matching(min_shift16)
    ctx.interpolate_frames(p, c, outs[0], FACTORS[0])
    single = ctx.last_level_match() if min_shift16 >= 0 else None
    ctx.interpolate_frames_multi(p, c, outs[1:], FACTORS[1:])
    got = [ctx.download(o) for o in outs]
    multi = ctx.last_level_match() if min_shift16 >= 0 else None
    return got, single, multi


def switch_off(ctx):
    ctx.set_level_matching(-1)
    restore(ctx)


@pytest.fixture(scope="module")
def scene_frames(ctx):
    made = {}

    def get(name):
        if name not in made:
            prev, curr = scene_of(name)[:2]
            h, w = prev.shape[:2]
            made[name] = (ctx.frame_from(prev), ctx.frame_from(curr), [ctx.create_frame(w, h) for _ in FACTORS])
        return made[name]

    yield get
    for p, c, outs in made.values():
        for f in [p, c] + outs:
            ctx.destroy_frame(f)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["faded", "pan32", "pan0", "static"])
def test_the_switch_equals_the_wrapper_around_the_chain(ctx, scene_frames, name, route):
    """Every route on every scene, through both entry points.  A static pair matches at every pixel, so no threshold fails it:
    that one combination does not exist.  Where the pair is inactive -- the pan at threshold 32, the static pair -- and at
    threshold 0 on the pan, whose map is the identity on every level a pixel has, the bytes are those of the same calls with
    the switch off, on the GPU itself."""
    r = ROUTES[route]
    prev, curr, threshold, m, _, chain = scene_of(name)
    if r.cut == "fails" and chain.fails is None:
        assert name == "static"
        return
    want, _ = expected(name, r, FACTORS)
    frames = scene_frames(name)
    try:
        got, single, multi = run_route(ctx, name, r, threshold, frames)
        off = run_route(ctx, name, r, -1, frames)[0] if name != "faded" else None
    finally:
        switch_off(ctx)
    assert single == multi == (m["shift_sum"], m["pixels"], bool(m["active"])), (single, multi)
    assert m["active"] == (name in ("faded", "pan0"))
    for t, g, e in zip(FACTORS, got, want):
        assert (g == e).all(), f"{name} {route} t={t}: {first_bad(g, e)}"
    if r.cut == "fails":                                 # the caller's own frames, byte for byte
        assert chain.is_cut(r)
        shown = [curr if t >= 0.5 else prev for t in FACTORS]
        assert all((g == s).all() for g, s in zip(got, shown))
    elif r.interpolator == "compensated" and r.generation == "interpolate":
        assert (got[-1] == curr).all()                   # t = 1 still gives curr exactly
    if off is not None:
        assert all((g == o).all() for g, o in zip(got, off)), f"{name} {route}: differs from the switch off"


def test_levelling_changes_the_faded_scene(ctx, scene_frames):
    """The tests above could pass on a switch that did nothing if the model's wrapper did nothing either: on the faded scene the
    levelled call differs from the plain one, and matches more pixels."""
    name, r = "faded", ROUTES["cut_passes"]
    prev, curr, threshold, _, seen, chain = scene_of(name)
    frames = scene_frames(name)
    try:
        on = run_route(ctx, name, r, threshold, frames)[0]
        levelled = ctx.last_pair_stats()[0]
        off = run_route(ctx, name, r._replace(cut=0), -1, frames)[0]
        plain = ctx.last_pair_stats()[0]
    finally:
        switch_off(ctx)
    assert any((a != b).any() for a, b in zip(on, off))
    assert levelled == chain.stats(r)
    print(f"matched per thousand: {pair.permille(plain)} as it is, {pair.permille(levelled)} levelled")
    assert pair.permille(plain) < 300 and pair.permille(levelled) > pair.permille(plain) + 2 * rc.ROOM


# ---- lanes, changing settings, changing sizes

def small_pairs():
    """Pairs of several sizes, faded and not: (prev, curr, min_shift16)."""
    out = []
    for k, (w, h) in enumerate([(64, 48), (96, 64), (40, 36), (64, 48), (33, 17), (96, 64)]):
        prev, curr = (lc.faded_pan if k % 2 == 0 else lc.pan)(w, h, 40 + k)
        out.append((prev, curr, (lc.THRESHOLD, 0, -1)[k % 3]))
    return out


def small_expected(prev, curr, threshold, t):
    chain = lambda p, c: rc.RouteChain(p, c).frames(rc.route(BASE), [t])
    if threshold < 0:
        return chain(prev, curr)[0], None
    frames, m = lm.wrapper(prev, curr, threshold, chain, [t])
    return frames[0], (m["shift_sum"], m["pixels"], bool(m["active"]))


def test_three_lanes_changing_switch_and_sizes_without_a_sync(ctx):
    """Six calls on three lanes, enqueued with no sync between them: the size changes under every lane's levelled frame, and the
    switch moves between 32, 0 and off from call to call.  Every output is the model's, and lfg_last_level_match of each lane
    is that of the lane's last levelling call."""
    pairs = small_pairs()
    t = 0.5
    want = [small_expected(p, c, s, t) for p, c, s in pairs]
    made, last = [], {}
    ctx.lanes(3)
    try:
        select(ctx, rc.RouteChain(pairs[0][0], pairs[0][1]), rc.route(BASE))
        for k, (prev, curr, threshold) in enumerate(pairs):
            ctx.lane_select(k % 3)
            h, w = prev.shape[:2]
            p, c, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h)
            ctx.set_level_matching(threshold)
            ctx.interpolate_frames(p, c, o, t)
            made.append((p, c, o))
            if threshold >= 0:
                last[k % 3] = want[k][1]
        ctx.sync()
        for lane, record in last.items():
            ctx.lane_select(lane)
            assert ctx.last_level_match() == record, lane
        for k, ((_, _, o), (frame, _)) in enumerate(zip(made, want)):
            got = ctx.download(o)
            assert (got == frame).all(), f"call {k}: {first_bad(got, frame)}"
    finally:
        for fs in made:
            for f in fs:
                ctx.destroy_frame(f)
        switch_off(ctx)


def test_a_fade_stream_pair_by_pair(ctx):
    """A 12-frame 96 x 64 stream that pans, fades out over its middle frames and fades back in, as a host would run it: every
    generated frame is the chain's under the wrapper, and the pairs the library reports as levelled are the model's."""
    frames = lc.fade_stream()
    h, w = frames[0].shape[:2]
    device = [ctx.frame_from(f) for f in frames]
    out = ctx.create_frame(w, h)
    levelled = wanted = 0
    try:
        select(ctx, rc.RouteChain(frames[0], frames[1]), rc.route(BASE))
        ctx.set_level_matching(lc.THRESHOLD)
        for k in range(1, len(frames)):
            ctx.interpolate_frames(device[k - 1], device[k], out, 0.5)
            got = ctx.download(out)
            want, record = small_expected(frames[k - 1], frames[k], lc.THRESHOLD, 0.5)
            assert (got == want).all(), f"pair {k}: {first_bad(got, want)}"
            assert ctx.last_level_match() == record
            levelled += ctx.last_level_match()[2]
            wanted += record[2]
    finally:
        for f in device + [out]:
            ctx.destroy_frame(f)
        switch_off(ctx)
    assert levelled == wanted == 6                       # the six pairs whose gain changes


# ---- argument errors

def test_argument_errors_return_invalid_and_the_next_call_is_right(ctx):
    lib, h = ctx.lib, ctx.h
    host = content(16, 8, 9)
    f, g = ctx.frame_from(host), ctx.create_frame(16, 8)
    other = ctx.create_frame(8, 8)
    mv = ctx.create_frame(16, 8, capi.FORMAT_MV_S8X2)
    rec, m = ctx.create_histogram_record(), ctx.create_levels_map()
    F, vp = ctypes.byref, ctypes.c_void_p
    odd = capi.Context.wrap(f.data + 2, 4, 4, capi.FORMAT_RGBA8, pitch=64)
    overlap = capi.Context.wrap(f.data + 64, 16, 7, capi.FORMAT_RGBA8, pitch=64)
    inf, nan = float("inf"), float("nan")
    bad = [
        lib.lfg_frame_histogram(h, None, 0, vp(rec.data)), lib.lfg_frame_histogram(h, F(f), 2, vp(rec.data)),
        lib.lfg_frame_histogram(h, F(f), 0, None), lib.lfg_frame_histogram(h, F(f), 0, vp(rec.data + 4)),
        lib.lfg_frame_histogram(h, F(mv), 0, vp(rec.data)), lib.lfg_frame_histogram(h, F(odd), 0, vp(rec.data)),
        lib.lfg_levels_match(h, None, vp(rec.data), 0, vp(m.data)), lib.lfg_levels_match(h, vp(rec.data), vp(rec.data), -1, vp(m.data)),
        lib.lfg_levels_match(h, vp(rec.data), vp(rec.data), 4081, vp(m.data)), lib.lfg_levels_match(h, vp(rec.data), vp(rec.data), 0, vp(m.data + 4)),
        lib.lfg_levels_match(h, vp(rec.data), vp(rec.data), 0, vp(rec.data + 8)), lib.lfg_levels_match(h, vp(rec.data), vp(rec.data), 0, None),
        lib.lfg_levels_apply(h, F(f), F(other), vp(m.data), 0, 0.0), lib.lfg_levels_apply(h, F(f), F(g), vp(m.data), 2, 0.0),
        lib.lfg_levels_apply(h, F(f), F(g), vp(m.data), 1, 1.5), lib.lfg_levels_apply(h, F(f), F(g), vp(m.data), 1, -0.1),
        lib.lfg_levels_apply(h, F(f), F(g), vp(m.data), 1, nan), lib.lfg_levels_apply(h, F(f), F(g), vp(m.data), 1, inf),
        lib.lfg_levels_apply(h, F(f), F(g), None, 0, 0.0), lib.lfg_levels_apply(h, F(f), F(mv), vp(m.data), 0, 0.0),
        lib.lfg_levels_apply(h, F(f), F(overlap), vp(m.data), 0, 0.0), lib.lfg_levels_apply(h, None, F(g), vp(m.data), 0, 0.0),
        lib.lfg_set_level_matching(h, -2), lib.lfg_set_level_matching(h, 4081),
    ]
    assert bad == [capi.ERR_INVALID] * len(bad), bad
    try:
        # the frame-taking calls with the switch on: nothing is enqueued, so no output byte changes
        ctx.lanes(2)
        ctx.lane_select(1)
        with pytest.raises(capi.LfgError):
            ctx.last_level_match()                           # this lane has made no levelling call
        ctx.set_level_matching(0)
        ctx.upload(g, np.full((8, 16, 4), 0x77, np.uint8))
        one = ctypes.c_float(0.5)
        outs = (ctypes.POINTER(capi.Frame) * 1)(ctypes.pointer(g))
        refused = [
            lib.lfg_interpolate_frames(h, F(f), F(other), F(g), 0.5), lib.lfg_interpolate_frames(h, F(f), F(f), F(other), 0.5),
            lib.lfg_interpolate_frames(h, F(f), F(f), F(g), 1.5), lib.lfg_interpolate_frames(h, F(f), F(f), F(g), nan),
            lib.lfg_interpolate_frames(h, F(f), F(f), F(f), 0.5), lib.lfg_interpolate_frames(h, None, F(f), F(g), 0.5),
            lib.lfg_interpolate_frames_multi(h, F(f), F(f), outs, ctypes.byref(one), 0),
            lib.lfg_interpolate_frames_multi(h, F(f), F(f), None, ctypes.byref(one), 1),
            lib.lfg_interpolate_frames_multi(h, F(f), F(f), outs, None, 1),
        ]
        assert refused == [capi.ERR_INVALID] * len(refused), refused
        with pytest.raises(capi.LfgError):
            ctx.last_level_match()                           # ... and still none
        assert (ctx.download(g) == 0x77).all()
        # a valid call after them gives the right bytes
        prev, curr = lc.faded_pan(16, 8, 3)
        ctx.upload(f, prev)
        c = ctx.frame_from(curr)
        select(ctx, rc.RouteChain(prev, curr), rc.route(BASE))
        ctx.set_level_matching(lc.THRESHOLD)
        ctx.interpolate_frames(f, c, g, 0.5)
        want, record = small_expected(prev, curr, lc.THRESHOLD, 0.5)
        assert (ctx.download(g) == want).all() and ctx.last_level_match() == record
        ctx.frame_histogram(f, rec)
        assert ctx.read_histogram_record(rec)[0] == 16 * 8
        ctx.destroy_frame(c)
    finally:
        switch_off(ctx)
        for x in (f, g, other, mv, rec, m):
            ctx.destroy_frame(x)
