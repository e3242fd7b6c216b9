"""The combined dispatch of lfg_interpolate_frames and lfg_interpolate_frames_multi -- all twelve context settings, the seven
opt-in switches among them -- against the CPU chain of tests/route_cases.py, byte for byte on every pixel: every combination of
the switches on one base setting, a hand-written cross of what that matrix fixes, switches changed between enqueued calls so
that every shared temporary changes hands, frame sizes that change under the routes' temporaries on one lane and on three, and
a default that never moved.  What the scene is held to, and that the chain is the per-feature models' own word:
tests/test_route_cases.py."""
import numpy as np
import pytest

from linux_fg_amd import capi
from tests import cases
from tests import route_cases as rc
from tests.gpu_kit import DEFAULT, apply, ctx, first_bad
from tests.test_gpu_dispatch import SIZES

pytestmark = pytest.mark.gpu

FACTORS = [cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS
GENERATION = {"interpolate": capi.GENERATION_INTERPOLATE, "extrapolate": capi.GENERATION_EXTRAPOLATE}


def select(ctx, chain, r):
    """The twelve setters a host calls for the route.  None of them waits for the GPU."""
    apply(ctx, r[:4], fused=r.fused, match_sad=r.match_sad, threshold=chain.threshold(r))
    ctx.set_generation(GENERATION[r.generation])
    ctx.set_static_protection(r.protect)
    ctx.set_bidirectional(r.bidirectional)
    ctx.set_half_resolution_motion(r.half_res)
    ctx.set_hole_reach(r.reach)
    ctx.set_subpixel_vectors(r.subpel)


def restore(ctx):
    ctx.lane_select(0)
    ctx.lanes(1)
    apply(ctx, DEFAULT)
    ctx.set_generation(capi.GENERATION_INTERPOLATE)
    for off in (ctx.set_static_protection, ctx.set_bidirectional, ctx.set_half_resolution_motion, ctx.set_hole_reach, ctx.set_subpixel_vectors):
        off(-1)


# ---- 1. and 2. the switch matrix and the cross, on the scene that tells the routes apart

@pytest.fixture(scope="module")
def scene(ctx):
    chain = rc.scene_chain()
    h, w = chain.prev.shape[:2]
    p, c = ctx.frame_from(chain.prev), ctx.frame_from(chain.curr)
    outs = [ctx.create_frame(w, h) for _ in FACTORS]
    yield chain, p, c, outs
    for f in [p, c] + outs:
        ctx.destroy_frame(f)


def check_route(ctx, scene, r):
    chain, p, c, outs = scene
    try:
        select(ctx, chain, r)
        ctx.interpolate_frames(p, c, outs[0], FACTORS[0])
        single = chain.threshold(r) >= 0 and ctx.last_pair_stats()
        ctx.interpolate_frames_multi(p, c, outs[1:], FACTORS[1:])
        got = [ctx.download(o) for o in outs]
        multi = chain.threshold(r) >= 0 and ctx.last_pair_stats()
    finally:
        restore(ctx)
    for t, g, e in zip(FACTORS, got, chain.frames(r, FACTORS)):
        assert (g == e).all(), f"{rc.route_id(r)} t={t}: {first_bad(g, e)}"
    if chain.threshold(r) >= 0:                                      # the record is taken on the final integer field
        assert single == multi == (chain.stats(r), r.cut == "fails"), rc.route_id(r)


@pytest.mark.parametrize("r", rc.matrix_routes(), ids=rc.route_id)
def test_every_combination_of_the_switches_equals_the_chain(ctx, scene, r):
    """3 x 2^6 combinations x both entry points.  The scene tells any two routes apart that the header defines differently
    (test_route_cases.py: test_routes_that_differ_give_different_frames), so a wrong precedence, a switch dropped on one branch
    or a field measured the wrong way fails here."""
    check_route(ctx, scene, r)


@pytest.mark.parametrize("r", rc.CROSS, ids=rc.route_id)
def test_the_cross_of_the_base_settings_equals_the_chain(ctx, scene, r):
    """What the matrix fixes: the shader under each switch, the fused order, the full search under the reference semantics,
    the other refinement radii, and the other values of every switch."""
    check_route(ctx, scene, r)


# ---- 3. switches changed between enqueued calls

# (route, factor).  Consecutive calls hand every shared temporary over: the key image between the 32-bit kinds and the 64-bit
# sub-pixel one (mc_keys / mcq_keys), the fill plane on and off (mc_fill), the backward fields used and unused (mv_bwd,
# mv_bwd_refined), the halves (half_prev, half_curr, mv_half), the refined field, the mask, the quarter-pixel field and the cut
# record; the fused flag alternates and match_sad moves.
SEQUENCE = [
    (rc.route(rc.BASE, bidirectional=1, half_res=1, reach=32, cut="passes"), 0.3),
    (rc.route(rc.BASE, subpel=1), 0.9),
    (rc.route(rc.BASE, protect=0, bidirectional=1, reach=32, half_res=1, fused=True), 0.5),
    (rc.route(rc.BASE, generation="extrapolate", cut="passes", reach=32), 5.0 / 6.0),
    (rc.route(("pyramid", -1, "compensated", 1), bidirectional=0, match_sad=300), 0.7),
    (rc.route(rc.BASE, subpel=2, half_res=2, cut="passes", fused=True), 0.3),
    (rc.route(rc.BASE, reach=255), 0.25),
    (rc.route(rc.SHADER, half_res=1, cut="passes", reach=32, bidirectional=1, subpel=1, protect=0, fused=True), 0.9),
    (rc.route(rc.BASE, protect=8, subpel=1), 0.3),
    (rc.route(rc.BASE, bidirectional=1, cut="fails"), 0.3),
    (rc.route(rc.BASE, bidirectional=1, reach=32, subpel=1), 0.3),
    (rc.route(rc.BASE, generation="extrapolate", half_res=1, cut="fails", fused=True), 0.3),
    (rc.route(rc.BASE), 0.7),
]


def test_switches_changed_between_enqueued_calls(ctx, scene):
    """One context, the setters between the calls, one sync at the end: output k is the chain under the route in force when
    call k was made.  Twice: in the second round every temporary exists, so the library has no reason to wait either."""
    chain, p, c, _ = scene
    h, w = chain.prev.shape[:2]
    want = [chain.frames(r, [t])[0] for r, t in SEQUENCE]
    assert len({e.tobytes() for e in want}) == len(SEQUENCE)         # a call that ran under a neighbour's route shows
    assert all(chain.is_cut(r) == (r.cut == "fails") for r, _ in SEQUENCE)
    kinds = [rc.effective(chain.resolved(r)).kind for r, _ in SEQUENCE]
    assert all(a != b for a, b in zip(kinds, kinds[1:])) and set(kinds) == set(rc.KINDS)
    last_record = [r for r, _ in SEQUENCE if r.cut != "off"][-1]
    outs = [ctx.create_frame(w, h) for _ in SEQUENCE]
    try:
        for rnd in range(2):
            for o in outs:
                ctx.upload(o, np.full((h, w, 4), 0x5A, np.uint8))
            for (r, t), o in zip(SEQUENCE, outs):
                select(ctx, chain, r)
                ctx.interpolate_frames(p, c, o, t)
            ctx.sync()
            for k, (o, e) in enumerate(zip(outs, want)):
                g = ctx.download(o)
                assert (g == e).all(), f"round {rnd} call {k} {rc.route_id(SEQUENCE[k][0])}: {first_bad(g, e)}"
            assert ctx.last_pair_stats() == (chain.stats(last_record), last_record.cut == "fails")
    finally:
        restore(ctx)
        for o in outs:
            ctx.destroy_frame(o)


# ---- 4. sizes that change under the routes' temporaries, on one lane and on three

# The route cycles call by call, so a lane's buffers are grown by one route and reused, smaller, by another.  The cut threshold
# is a number here, and the model decides: the scenes of a few pixels are no match at all.
THRESHOLD = 300
HEAVY = [
    rc.route(rc.BASE, bidirectional=1, half_res=1, reach=32, cut=THRESHOLD),
    rc.route(rc.BASE, protect=0, reach=32, half_res=1),
    rc.route(rc.BASE, subpel=1, half_res=1),
    rc.route(rc.BASE, generation="extrapolate", cut=THRESHOLD),
]
SINGLE, MULTI = 0.3, [0.9, 0.25, 5.0 / 6.0]
_chains = {}


def small_chain(w, h, k):
    if (w, h, k) not in _chains:
        _chains[(w, h, k)] = rc.RouteChain(*cases.small_scene(w, h, 70 + k))
    return _chains[(w, h, k)]


def run_sizes(ctx, lanes, offset):
    """Pair k of its own size and content on lane k % lanes under HEAVY[(k + offset) % 4], its own buffers, both entry points;
    everything is enqueued before the one sync.  Returns [(chain, route, frames at SINGLE and MULTI, the lane's record then)]."""
    chains = [small_chain(w, h, k) for k, (w, h) in enumerate(SIZES)]
    routes = [HEAVY[(k + offset) % len(HEAVY)] for k in range(len(SIZES))]
    frames = []
    try:
        for ch in chains:
            h, w = ch.prev.shape[:2]
            frames.append((ctx.frame_from(ch.prev), ctx.frame_from(ch.curr), [ctx.create_frame(w, h) for _ in range(1 + len(MULTI))]))
        ctx.lanes(lanes)
        for k, ((p, c, outs), ch, r) in enumerate(zip(frames, chains, routes)):
            ctx.lane_select(k % lanes)
            select(ctx, ch, r)
            ctx.interpolate_frames(p, c, outs[0], SINGLE)
            ctx.interpolate_frames_multi(p, c, outs[1:], MULTI)
        ctx.sync()
        return [(ch, r, [ctx.download(o) for o in outs]) for ch, r, (_, _, outs) in zip(chains, routes, frames)]
    finally:
        restore(ctx)
        for p, c, outs in frames:
            for f in [p, c] + outs:
                ctx.destroy_frame(f)


@pytest.mark.parametrize("offset", [0, 2])
def test_sizes_that_change_under_the_routes_temporaries(ctx, offset):
    """One lane, then the same sequence with frames in flight on three: every output is the chain of its own pair and route."""
    assert max(w for w, _ in SIZES) <= 257 and max(h for _, h in SIZES) <= 131 and (1, 1) in SIZES
    for lanes in (1, 3):
        passed = 0
        for k, (ch, r, got) in enumerate(run_sizes(ctx, lanes, offset)):
            for t, g, e in zip([SINGLE] + MULTI, got, ch.frames(r, [SINGLE] + MULTI)):
                assert (g == e).all(), f"{rc.route_id(r)} lanes={lanes} pair {k} {SIZES[k]} t={t}: {first_bad(g, e)}"
            passed += r.cut != "off" and not ch.is_cut(r)
        assert passed >= 3                                           # most pairs pass the threshold: the routes run, not the fallback


# ---- 5. a default that never moved

def test_restored_context_equals_a_fresh_one(ctx, scene):
    """Last in the file: the context that went through every route above -- and, so that it holds when run alone, through
    four heavy ones once more here -- with all twelve setters put back, against a context that touched no setter at all, and
    both against the chain of the default setting."""
    chain, p, c, outs = scene
    try:
        for r in (SEQUENCE[0][0], SEQUENCE[1][0], SEQUENCE[2][0], SEQUENCE[3][0]):
            select(ctx, chain, r)
            ctx.interpolate_frames(p, c, outs[0], 0.7)
            ctx.interpolate_frames_multi(p, c, outs[1:], FACTORS[1:])
    finally:
        restore(ctx)
    used = []
    for t, o in zip(FACTORS, outs):
        ctx.interpolate_frames(p, c, o, t)
        used.append(ctx.download(o))
    h, w = chain.prev.shape[:2]
    with capi.Context(0) as fresh:
        fp, fc, fo = fresh.frame_from(chain.prev), fresh.frame_from(chain.curr), fresh.create_frame(w, h)
        for t, u, e in zip(FACTORS, used, chain.frames(rc.route(DEFAULT), FACTORS)):
            fresh.interpolate_frames(fp, fc, fo, t)
            g = fresh.download(fo)
            assert (u == g).all(), f"t={t}: the used context differs from a fresh one: {first_bad(u, g)}"
            assert (g == e).all(), f"t={t}: {first_bad(g, e)}"
        assert (chain.frames(rc.route(DEFAULT), FACTORS)[0] == cases.Chain(chain.prev, chain.curr).frames(DEFAULT, FACTORS)[0]).all()
