"""lfg_motion held to its model while a communicator exists (a one-rank communicator, as in tests/test_gpu_comm.py).

Under a communicator lfg_restream re-creates every lane's stream under a CU mask and the persistent grid is cut to what the other
CUs hold (persistent_grid_most): the default configuration of the N > 1 step.  tests/test_gpu_comm.py checks the mask, the
ordering and that a broadcast finds a CU; here the VECTORS of such a context are compared with their reference, for every
reservation LFG_COMM_CUS accepts, with one lane and with three, and again after lfg_comm_destroy.  The expected grids come from
motion_plan() before lfg_comm_init and from comm_reserved_cus().  LFG_PREF_GROUPS is never set here (tests/test_gpu_launch_geometry.py).
And lfg_comm_init / lfg_comm_destroy in the middle of a session: lanes with work enqueued, a cut record with its event, marks, and
an adopted stream beside own streams, against the chain of tests/route_cases.py."""
import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import geometry_cases as gc
from tests.gpu_kit import ctx, first_bad                                    # noqa: F401 (ctx is this module's fixture)
from tests.test_gpu_launch_geometry import Loaded, check_pair, device_grids, knob_context, literal, reference

pytestmark = pytest.mark.gpu

# the mixed pairs and the hand-over pair at 616 x 448 -- and the hand-over pair at the size where segments do go through the
# run-time queue (tests/geometry_cases.py, QUEUE_SIZE)
CASES = [(gc.HAND_OVER_SIZE, f"mixed {seed}") for seed in gc.MIXED_SEEDS] + [(gc.HAND_OVER_SIZE, "hand-over"), (gc.QUEUE_SIZE, "hand-over")]
LABELS = [f"{name} at {size[0]} x {size[1]}" for size, name in CASES] + ["3840 x 2160"]


@pytest.fixture(scope="module")
def uhd(ctx):
    """test_a_broadcast_finds_a_cu_while_a_full_persistent_grid_runs' first input at its upscaled size, 3840 x 2160 -- a pan under
    sensor noise of +-8 levels, both frames through lfg_scale: the one size here whose plan has more units than the grid has
    workgroups without a knob -- and the literal kernel's vectors on it."""
    w, h = 1920, 1080
    prev = synth.make_prev(w, h, seed=811)
    noise = synth.noise_bytes(w, h, 861) % 17
    curr = np.clip(synth.translate(prev, (3, -2), 811).astype(np.int16) + noise.astype(np.int16) - 8, 0, 255).astype(np.uint8)
    ups = []
    for x in (prev, curr):
        f, up = ctx.frame_from(x), ctx.create_frame(2 * w, 2 * h)
        ctx.scale(f, up)
        ups.append(ctx.download(up))
        ctx.destroy_frame(f); ctx.destroy_frame(up)
    want = literal(ctx, ("uhd", "pan under noise"), ups[0], ups[1], "reference")
    inner = want[40:-40, 40:-40]
    assert (inner[..., 0] == -6).mean() > 0.99 and (inner[..., 1] == 4).mean() > 0.99      # (the pan is found: the input is what it says)
    return ups[0], ups[1], want


def run_one_lane(ctx, c, what, uhd):
    for size, name in CASES:
        check_pair(ctx, c, what, size, name, gc.pairs_of(size)[name][2])
    big = Loaded(c, uhd[0], uhd[1])
    for call in range(2):
        got = big.vectors()
        assert (got == uhd[2]).all(), f"{what}: 3840 x 2160, call {call}: {first_bad(got, uhd[2])}"
    big.free()


def run_three_lanes(ctx, c, what, uhd, rounds=2):
    """The small pairs and the large one on lanes 0, 1, 2, 0, 1, 2, enqueued back to back, `rounds` times before the one sync:
    from the second round on a lane's launch goes by the verdict of its first."""
    c.lanes(3)
    try:
        pairs = [Loaded(c, *gc.pairs_of(size)[name][:2]) for size, name in CASES] + [Loaded(c, uhd[0], uhd[1])]
        want = [reference(ctx, size, name, "reference") for size, name in CASES] + [uhd[2]]
        mvs = [[c.create_frame(p.w, p.h, capi.FORMAT_MV_S8X2) for p in pairs] for _ in range(rounds)]
        c.sync()
        for r in range(rounds):
            for k, pair in enumerate(pairs):
                c.lane_select(k % 3)
                c.motion(pair.p, pair.q, mvs[r][k])
        c.sync()
        for r in range(rounds):
            for k, w in enumerate(want):
                got = c.download(mvs[r][k])
                assert (got == w).all(), f"{what}, three lanes, round {r}, {LABELS[k]} on lane {k % 3}: {first_bad(got, w)}"
        c.lane_select(0)
        for f in [f for row in mvs for f in row]:
            c.destroy_frame(f)
        for p in pairs:
            p.free()
    finally:
        c.lane_select(0)
        c.lanes(1)


@pytest.mark.parametrize("cus", gc.COMM_CUS)
def test_motion_equals_its_reference_under_every_reservation(ctx, uhd, monkeypatch, cus):
    with knob_context(monkeypatch, dict(LFG_COMM_CUS=str(cus))) as c:
        slots, device_cus = device_grids(c)
        before = c.motion_plan()
        assert before[1] == slots
        c.comm_init(1, 0, capi.Context.comm_unique_id())
        reserved = c.comm_reserved_cus()
        assert reserved == cus
        grid = slots // device_cus * (device_cus - reserved)
        assert c.motion_plan() == (before[0], grid) and 0 < grid < slots
        run_one_lane(ctx, c, f"{cus} CUs kept", uhd)
        run_three_lanes(ctx, c, f"{cus} CUs kept", uhd)
        c.comm_destroy()
        assert c.comm_reserved_cus() == 0 and c.motion_plan() == before
        run_one_lane(ctx, c, f"{cus} CUs given back", uhd)
        run_three_lanes(ctx, c, f"{cus} CUs given back", uhd)


# ------------------------------------------------------------------ lfg_comm_init / lfg_comm_destroy in mid-session

def _mid_session_chains():
    """Lane 0: the scene under BASE; lane 1: the scene reversed under BASE + bidirectional + reach 32; lane 2 (on an adopted stream):
    the scene under that route with a threshold it fails -- three records or verdicts that differ, so a lane that answered with
    another lane's would show."""
    from tests import route_cases as rc
    prev, curr = rc.route_scene()
    both = rc.route(rc.BASE, bidirectional=1, reach=32, cut="passes")
    plan = [(rc.RouteChain(prev, curr), rc.route(rc.BASE, cut="passes")), (rc.RouteChain(curr, prev), both), (None, both._replace(cut="fails"))]
    plan[2] = (plan[0][0], plan[2][1])
    for chain in (plan[0][0], plan[1][0]):
        chain.passes, chain.fails = rc.thresholds(chain, [rc.route(rc.BASE, cut="passes"), both])
    return plan


def test_a_communicator_comes_and_goes_while_every_lane_has_work(ctx, monkeypatch):
    """lfg_comm_init and lfg_comm_destroy re-create every lane's OWN stream (lfg_restream: under the CU mask, and back), and
    synchronise those streams themselves.  Three lanes, lane 2 on a stream the caller owns; every lane is given an
    lfg_interpolate_frames_multi with cut detection on and the communicator is created -- later destroyed -- with no sync in
    between.  Held: the frames equal the CPU chain; lfg_last_pair_stats answers with each lane's own record and verdict, taken
    before its stream went; a mark set before the change is still waited for and a mark on the new stream orders a dependent
    call behind a long one; the own lanes' handles are new, the adopted one is the caller's; a second round under the mask
    equals the chain again."""
    from tests import cases
    from tests.order_runner import Hip
    from tests.test_gpu_routes import restore, select
    plan = _mid_session_chains()
    factors = cases.MATRIX_FACTORS
    want = [chain.frames(r, factors) for chain, r in plan]
    records = [(chain.stats(r), chain.is_cut(r)) for chain, r in plan]
    assert [cut for _, cut in records] == [False, False, True] and records[0][0] != records[1][0]
    h, w = plan[0][0].prev.shape[:2]
    old, new = synth.make_prev(w, h, seed=7401), synth.make_prev(w, h, seed=7402)
    scaled = {}
    for name, x in (("old", old), ("new", new)):                                # what lfg_scale gives on an idle default context
        f, up = ctx.frame_from(x), ctx.create_frame(2 * w, 2 * h)
        ctx.scale(f, up)
        scaled[name] = ctx.download(up)
        ctx.destroy_frame(f); ctx.destroy_frame(up)
    long_a, long_b = gc.noise_pair(gc.HAND_OVER_SIZE)                           # a call of a millisecond or more: every segment searched in full
    hip = Hip()
    S = hip.stream()
    with knob_context(monkeypatch, {}) as c:
        try:
            c.lanes(3)
            c.lane_select(2)
            c.set_stream(S)
            scenes = [(c.frame_from(chain.prev), c.frame_from(chain.curr)) for chain, _ in plan]
            outs = [[c.create_frame(w, h) for _ in factors] for _ in plan]
            F, F2 = c.frame_from(old), c.frame_from(new)
            U, U2, G, G2 = (c.create_frame(2 * w, 2 * h) for _ in range(4))
            blocker = Loaded(c, long_a, long_b)
            device_grids(c)                                                     # (the slots are asked of the runtime when first needed)
            plan_before = c.motion_plan()

            def handles():
                out = []
                for lane in range(3):
                    c.lane_select(lane)
                    out.append(c.get_stream())
                return out

            def enqueue_every_lane():
                for o in [o for lane in outs for o in lane] + [U, U2, G, G2]:
                    c.upload(o, np.full((o.height, o.width, 4), 0x5A, np.uint8))
                for lane, (chain, r) in enumerate(plan):
                    c.lane_select(lane)
                    select(c, chain, r)
                    c.interpolate_frames_multi(*scenes[lane], outs[lane], factors)
                c.lane_select(0)
                c.motion(blocker.p, blocker.q, blocker.mv)
                c.scale(F, U)
                c.lane_mark()                                                   # ... on the stream that is about to go

            def held(what, before):
                after = handles()
                assert after[2] == before[2] == S, what
                assert after[0] != before[0] and after[1] != before[1] and len(set(after)) == 3, (what, before, after)
                # the mark from before the change: lane 1 waits for it (nothing left to wait for) and reads what lane 0 wrote
                c.lane_select(1)
                c.lane_wait(0)
                c.copy(U, G)
                # a mark on the NEW stream, behind a long call: the dependent copy on lane 1 has to wait for it
                c.lane_select(0)
                c.motion(blocker.p, blocker.q, blocker.mv)
                c.scale(F2, U2)
                c.lane_mark()
                c.lane_select(1)
                c.lane_wait(0)
                c.copy(U2, G2)
                c.lane_sync()                                                   # lane 1 alone
                assert (c.download(G2) == scaled["new"]).all(), f"{what}: the copy ran ahead of the mark on the new stream"
                assert (c.download(G) == scaled["old"]).all(), f"{what}: the mark from before the change"
                c.sync()
                for lane, (chain, r) in enumerate(plan):
                    c.lane_select(lane)
                    assert c.last_pair_stats() == records[lane], (what, lane)
                    for t, o, e in zip(factors, outs[lane], want[lane]):
                        g = c.download(o)
                        assert (g == e).all(), f"{what}, lane {lane}, t={t}: {first_bad(g, e)}"
                return after

            at = handles()
            enqueue_every_lane()
            c.comm_init(1, 0, capi.Context.comm_unique_id())                    # no sync in between
            reserved = c.comm_reserved_cus()
            assert reserved > 0 and c.motion_plan()[1] < plan_before[1]
            at = held("lfg_comm_init in mid-session", at)
            enqueue_every_lane()                                                # a second round, on the masked streams
            c.sync()
            assert handles() == at
            for lane in range(3):
                c.lane_select(lane)
                assert c.last_pair_stats() == records[lane], lane
                for t, o, e in zip(factors, outs[lane], want[lane]):
                    g = c.download(o)
                    assert (g == e).all(), f"second round under the mask, lane {lane}, t={t}: {first_bad(g, e)}"
            enqueue_every_lane()
            c.comm_destroy()                                                    # likewise
            assert c.comm_reserved_cus() == 0 and c.motion_plan() == plan_before
            held("lfg_comm_destroy in mid-session", at)
        finally:
            c.sync()
            c.lane_select(2)
            c.set_stream(None)
            restore(c)
    assert hip.rt.hipStreamQuery(S) == 0 and hip.rt.hipStreamDestroy(S) == 0    # the adopted stream was the caller's throughout


# ------------------------------------------------------------------ every other frame-taking call on a masked stream

# tests/test_gpu_big_views.py's table of calls: each with the inputs, the call and the CPU model its own test file holds it to
MASKED_CALLS = ["scale_generic", "resample_up", "resample_antiring", "sharpen", "nv12_to_rgba_left", "rgba_to_nv12_left",
                "frame_diff", "frame_ssim", "pair_match", "hole_fill_plane", "motion_pyramid", "motion_refine", "motion_expand", "motion_subpel"]


@pytest.fixture(scope="module")
def masked():
    """A context whose streams leave 8 CUs to a communicator."""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("LFG_COMM_CUS", raising=False)
        c = capi.Context(0)
    try:
        c.comm_init(1, 0, capi.Context.comm_unique_id())
        assert c.comm_reserved_cus() == 8
        yield c
        c.sync()
        c.comm_destroy()
    finally:
        c.close()


@pytest.mark.parametrize("name", MASKED_CALLS)
def test_the_call_equals_its_model_on_a_masked_stream(masked, name):
    """Not a second kernel suite: one call each at tests/big_views.py's small image, every operand an ordinary frame -- the grids
    that are sized from the device's CU count have to be right where the stream may use 8 CUs fewer."""
    from tests import big_views as bv
    from tests import test_gpu_big_views as calls
    calls._run_case(masked, None, name, None, "ordinary", *bv.IMAGE)


def test_scale_2x_equals_the_f64_model_on_a_masked_stream(masked):
    """(the table's own 2x entry expects the generic kernel, as a view of 2 GiB takes it: here the exact-2x kernel has to run)"""
    from oracle import scale_f64 as f64
    from tests.test_gpu_parity import _scale_checked
    w, h = next(wh for wh in f64.sweep_2x_shapes() if wh[0] > 480 and wh[1] > 16)       # more than one workgroup across, more than one strip
    _scale_checked(masked, f64.contents(w, h, seed=1000 * w + h)["noise"], 2 * w, 2 * h, 1, f"2x {w}x{h} on a masked stream")


def test_upscale_edge_equals_its_model_on_a_masked_stream(masked):
    from tests import test_gpu_upscale_edge as ue
    w, h, ow, oh = ue.SHAPES[4]
    for name, frame in ue.inputs(w, h):
        got, want = ue.gpu(masked, frame, ow, oh), ue.model(frame, ow, oh)
        assert (got == want).all(), f"{name}: {first_bad(got, want)}"
