"""lfg_motion's prefiltered path held to its model under every launch geometry (tests/geometry_cases.py has the pairs and rows).

The persistent prefilter kernel's workgroups draw plan units, hand segments over through a queue, may come to own a queue slot
nobody has filled yet, and poll until the last plan unit is done: what a workgroup does depends on how many the launch has.
By default the grid is min(units, slots), so below 4K every unit has a workgroup of its own and the loop "finish a unit, draw the
next one, then turn to the queue" never runs a second time.  LFG_PREF_GROUPS sets the grid directly -- to the
values shipped configurations reach (5/8 of the slots with frames in flight; what a communicator's reservation leaves; the smaller
of the two), which no test reaches on purpose, and to 1, 3, 8 and 37, where every workgroup takes many units at frame sizes a
test can afford.  The run-time queue is in use at 940 x 1000 alone (tests/geometry_cases.py says why): lfg_motion_hand_over_stats
is the evidence, not the count of open segments, which the shared tiles' segments raise as well.  LFG_RESOLVE_GROUPS and LFG_DYN_PARTS_RT do the same for the resolve kernel's grid and the parts of a
handed-over segment.  Every comparison is of integer vectors or bytes, bit for bit.

Why any grid of at least one workgroup ends (csrc/motion_prefilter.hip, motion_prefilter_kernel; read before these rows were run):
  * Thread 0 of a workgroup waits in two places only.  wait_entry(h) is called for a slot h < min(queueCount, cap) alone: the
    pusher has already counted the slot, its entry is an atomic store away, and the pusher needs nothing from the waiting workgroup.
  * The loop at "Out of plan units" is entered with an owned slot only, after the fetch-and-add on ctrl[kCtrlNextUnit] returned
    an index >= planUnits -- so every plan unit has been DRAWN, each by a workgroup that has started and is running it or has
    finished it.  A unit's run does not wait for anybody (one barrier among its own four waves), so ctrl[kCtrlUnitsDone] reaches
    planUnits whatever the other workgroups do, and the loop leaves: with the slot's entry if the slot was pushed (a push
    precedes its unit's count), without it otherwise.  Only a running plan unit can push, so nothing is pushed afterwards.
  * No wait is for a workgroup that has not started: a grid larger than the device holds at once would still end, a grid of one
    is the simplest case -- the workgroup draws every unit itself, then takes the slots below queueCount in turn, and when its
    slot is past queueCount finds ctrl[kCtrlUnitsDone] == planUnits at the first poll.
  * No segment is left behind: slots are handed out in order by fetch-and-add, a workgroup that gives its slot up has seen
    every plan unit counted and queueCount <= its slot, and pushes beyond `cap` are not made (the segment is searched in place).
  * As shipped (lfg_motion_tune.hpp: LFG_QUEUE_FIRST false) a workgroup looks at the queue only once the plan has no unit left for
    it, so "keep an owned slot through a further plan unit" is compiled out and `owned` is set in the out-of-units branch alone;
    the argument above does not depend on it.  What a small grid changes is how many units a workgroup runs before it gets there,
    and how many workgroups are left to share the queue's entries: one, at a grid of one.
The resolve kernel loops over its rows by grid stride and waits for nobody.  LFG_PREF_GROUPS is never combined with a
communicator here: above motion_plan()[1] that is not a configuration the library ships."""
import contextlib

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import geometry_cases as gc
from tests.gpu_kit import ctx, first_bad                                    # noqa: F401 (ctx is this module's fixture)

pytestmark = pytest.mark.gpu

KNOBS = ("LFG_PREF_GROUPS", "LFG_RESOLVE_GROUPS", "LFG_DYN_PARTS_RT", "LFG_TIER_FORCE", "LFG_LEAN_FORCE", "LFG_MOTION_STRIP",
         "LFG_MOTION_HINTS", "LFG_MOTION_LEAN", "LFG_MOTION_MODE", "LFG_MOTION_RIM_SPLIT", "LFG_FUSED_MOTION_INTERPOLATE", "LFG_FALLBACK_FULL",
         "LFG_COMM_CUS")
SEMANTICS = {"reference": capi.SEMANTICS_REFERENCE, "intended": capi.SEMANTICS_INTENDED}
REPLAN_PAIR = ((300, 200), "mixed 9117")       # run between two pairs of another size: the workspace is planned again


@contextlib.contextmanager
def knob_context(monkeypatch, env, lanes=1):
    """A fresh context under `env` and none of the other knobs (they are read when it is created)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = capi.Context(0)
    try:
        if lanes > 1:
            c.lanes(lanes)
        yield c
    finally:
        c.close()


def device_grids(c):
    """(slots, CUs) of the device from a context without a communicator."""
    c.motion_workspace_size(64, 64)             # (the slots are asked of the runtime when first needed)
    assert c.comm_reserved_cus() == 0
    cus = sum(bin(word).count("1") for word in c.comm_cu_mask())
    return c.motion_plan()[1], cus


class Loaded:
    """A pair on the device with a vector frame of its own."""

    def __init__(self, c, prev, curr):
        self.c, (self.h, self.w) = c, prev.shape[:2]
        self.p, self.q = c.frame_from(prev), c.frame_from(curr)
        self.mv = c.create_frame(self.w, self.h, capi.FORMAT_MV_S8X2)

    def vectors(self, semantics="reference", mode=capi.MOTION_PREFILTERED):
        c = self.c
        c.set_semantics(SEMANTICS[semantics]); c.set_motion_mode(mode)
        try:
            c.upload(self.mv, np.full((self.h, self.w, 2), 0x5A, np.int8))      # (every vector has to be written)
            c.motion(self.p, self.q, self.mv)
            return c.download(self.mv)
        finally:
            c.set_semantics(capi.SEMANTICS_REFERENCE); c.set_motion_mode(capi.MOTION_PREFILTERED)

    def free(self):
        for f in (self.p, self.q, self.mv):
            self.c.destroy_frame(f)


_literal = {}


def literal(ctx, key, prev, curr, semantics):
    """The literal kernel's vectors on the default context, once per session."""
    if (key, semantics) not in _literal:
        pair = Loaded(ctx, prev, curr)
        _literal[key, semantics] = pair.vectors(semantics, capi.MOTION_EXACT_ONLY)
        _literal[key, semantics].setflags(write=False)
        pair.free()
    return _literal[key, semantics]


def reference(ctx, size, name, semantics):
    """What lfg_motion has to give on pairs_of(size)[name]: the oracle at the two small sizes, the literal kernel -- which
    tests/test_gpu_parity.py holds to the oracle -- above."""
    if size in gc.ORACLE_SIZES:
        return gc.oracle_vectors(size, name, semantics)
    prev, curr, _ = gc.pairs_of(size)[name]
    return literal(ctx, (size, name), prev, curr, semantics)


def all_cases():
    """(size, name, semantics) of every pair of every size, name-major: two neighbours never share a size."""
    names = [f"mixed {seed}" for seed in gc.MIXED_SEEDS] + ["noise", "scattered", "hand-over"]
    cases = [(size, name, gc.pairs_of(size)[name][2]) for name in names for size in gc.ALL_SIZES if name in gc.pairs_of(size)]
    assert all(a[0] != b[0] for a, b in zip(cases, cases[1:])) and len(cases) == sum(len(gc.pairs_of(size)) for size in gc.ALL_SIZES)
    return cases


def is_fade(size, name):
    return name.startswith("mixed ") and gc.has_fade(size, int(name.split()[1]))


def check_pair(ctx, c, row, size, name, semantics, calls=2, tier=None):
    """The pair under each of its tie orders on context c, `calls` times in a row, against the reference -- with the evidence that
    the mechanism the pair is there for did run."""
    prev, curr, _ = gc.pairs_of(size)[name]
    pair = Loaded(c, prev, curr)
    try:
        for sem in semantics:
            want = reference(ctx, size, name, sem)
            for call in range(calls):
                got = pair.vectors(sem)
                assert (got == want).all(), f"{row}: {name} at {size[0]}x{size[1]}, {sem} order, call {call}: {first_bad(got, want)}"
                if name == "hand-over":
                    assert c.motion_open_segments()[0] > 0, (row, name, size)
                if size == gc.QUEUE_SIZE:                          # whole tiles: segments without a match go through the queue ...
                    asked, room = c.motion_hand_over_stats()
                    assert asked > 0 and room > 0, (row, name, asked, room)
                    if name == "hand-over":                        # ... and on this pair more of them ask than it holds
                        assert asked > room, (row, name, asked, room)
                    if name == "scattered":                        # ... on this one fewer, one by one: every one goes through it
                        assert asked <= room // 2, (row, name, asked, room)
                else:                                              # (every tile shared between units: nothing is handed over)
                    assert c.motion_hand_over_stats()[0] == 0, (row, name, size)
                if is_fade(size, name):
                    assert c.motion_last_stats()[1] > 0, (row, name, size, sem)
                if tier is not None:
                    assert c.motion_last_variant() == tier, (row, name, size)
    finally:
        pair.free()


# ------------------------------------------------------------------ the references, and the pairs' mechanisms without a knob

SMALL_CASES = [(size, name, sem) for size in gc.ORACLE_SIZES for name, (_, _, runs) in gc.pairs_of(size).items() for sem in runs]


@pytest.mark.parametrize("size,name,semantics", SMALL_CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else v)
def test_the_literal_kernel_is_the_oracle_on_the_small_pairs(ctx, size, name, semantics):
    prev, curr, _ = gc.pairs_of(size)[name]
    want = gc.oracle_vectors(size, name, semantics)
    got = literal(ctx, (size, name), prev, curr, semantics)
    assert (got == want).all(), first_bad(got, want)


def test_the_pairs_show_their_mechanisms_on_a_default_context(ctx, monkeypatch):
    """Conditions on the INPUTS, checked where no knob is set: a row that fails them afterwards names the knob, this the pair."""
    slots, cus = device_grids(ctx)
    assert slots > max(gc.SMALL_GRIDS) and cus > max(gc.COMM_CUS), (slots, cus)
    assert all(0 < g < slots for g in gc.shipped_grids(slots, cus).values())
    for size, name, semantics in all_cases():
        check_pair(ctx, ctx, "no knob", size, name, semantics, calls=1, tier=0)
    assert sum(is_fade(size, name) for size, name, _ in all_cases()) >= len(gc.SIZES)
    with knob_context(monkeypatch, dict(LFG_TIER_FORCE="1")) as c:
        check_pair(ctx, c, "tier alone", gc.SIZES[2], "mixed 9117", ("reference",), calls=1, tier=1)
    with knob_context(monkeypatch, dict(LFG_LEAN_FORCE="1"), lanes=2) as c:
        for name, (prev, curr) in gc.lean_pairs().items():
            pair = Loaded(c, prev, curr)
            got, want = pair.vectors(), literal(ctx, ("lean", name), prev, curr, "reference")
            used, listed, _ = c.motion_lean_stats()
            assert used and listed > 50, (name, used, listed)
            assert (got == want).all(), f"lean alone, {name}: {first_bad(got, want)}"
            pair.free()
    with knob_context(monkeypatch, dict(LFG_MOTION_STRIP="1")) as c:
        name, prev, curr, shift = gc.strip_pair()
        pair = Loaded(c, prev, curr)
        got, want = pair.vectors(), literal(ctx, ("strip", name), prev, curr, "reference")
        assert c.motion_strip_stats() == (prev.shape[0], prev.shape[1]), (name, c.motion_strip_stats())
        assert (got == want).all(), f"strip alone, {name}: {first_bad(got, want)}"
        pair.free()


# ------------------------------------------------------------------ the rows

@pytest.mark.parametrize("row", gc.ROW_NAMES)
def test_motion_equals_its_reference_under_the_row(ctx, monkeypatch, row):
    """Every pair the row's kind runs, under both tie orders where the pair has them, twice in a row on one context (the workspace
    and the control area the hint kernel clears are reused) and always behind a pair of another size (the workspace is planned
    again)."""
    env, kind = gc.knob_rows(*device_grids(ctx))[row]
    tier = 1 if env.get("LFG_TIER_FORCE") == "1" else 0
    if kind == "all":
        with knob_context(monkeypatch, env) as c:
            for size, name, semantics in all_cases():
                check_pair(ctx, c, row, size, name, semantics, tier=tier)
        return
    with knob_context(monkeypatch, env, lanes=2 if kind == "lean" else 1) as c:
        if kind == "lean":
            cases = [(("lean", name), prev, curr) for name, (prev, curr) in gc.lean_pairs().items()]
        else:
            name, prev, curr, _ = gc.strip_pair()
            cases = [(("strip", name), prev, curr)]
        for lane in range(c.lane_count()):
            c.lane_select(lane)
            for key, prev, curr in cases:
                pair = Loaded(c, prev, curr)
                for sem in ("reference", "intended"):
                    want = literal(ctx, key, prev, curr, sem)
                    for call in range(2):
                        got = pair.vectors(sem)
                        assert (got == want).all(), f"{row}: {key[1]}, lane {lane}, {sem} order, call {call}: {first_bad(got, want)}"
                        if kind == "lean":
                            assert c.motion_lean_stats()[0], (row, key, lane)
                        else:
                            assert c.motion_strip_stats() != (0, 0), (row, key)
                pair.free()
                check_pair(ctx, c, row, *REPLAN_PAIR, ("reference",), calls=1)      # another size in between
        c.lane_select(0)


# ------------------------------------------------------------------ lanes

@pytest.mark.parametrize("grid", ["five eighths", 3])
@pytest.mark.parametrize("lanes", [2, 3])
def test_lanes_under_a_cut_grid_each_give_their_pairs_reference(ctx, monkeypatch, lanes, grid):
    """Frames in flight: a handed-over segment in 4 parts, the resolve kernel on its large grid, the lanes' persistent launches
    beside each other -- each lane a different pair, enqueued back to back without a sync, three rounds."""
    slots, cus = device_grids(ctx)
    groups = gc.shipped_grids(slots, cus)[grid] if isinstance(grid, str) else grid
    cases = [(gc.QUEUE_SIZE, "hand-over"), (gc.QUEUE_SIZE, "scattered"), (gc.HAND_OVER_SIZE, "noise")][:lanes]
    want = [reference(ctx, size, name, "reference") for size, name in cases]
    rounds = 3
    with knob_context(monkeypatch, dict(LFG_PREF_GROUPS=str(groups)), lanes=lanes) as c:
        pairs = [Loaded(c, *gc.pairs_of(size)[name][:2]) for size, name in cases]
        mvs = [[c.create_frame(p.w, p.h, capi.FORMAT_MV_S8X2) for p in pairs] for _ in range(rounds)]
        c.sync()
        for r in range(rounds):
            for lane, pair in enumerate(pairs):
                c.lane_select(lane)
                c.motion(pair.p, pair.q, mvs[r][lane])
        c.sync()
        for r in range(rounds):
            for lane, (size, name) in enumerate(cases):
                got = c.download(mvs[r][lane])
                assert (got == want[lane]).all(), f"{lanes} lanes, {groups} workgroups, round {r}, lane {lane} ({name}): {first_bad(got, want[lane])}"
        c.lane_select(0)
        asked, room = c.motion_hand_over_stats()
        assert asked > room // 2 > 0, (asked, room)                             # lane 0's pair: more than the queue holds in 4 parts a segment


# ------------------------------------------------------------------ the fused order

def test_fused_order_on_three_workgroups_gives_the_unfused_bytes(ctx, monkeypatch):
    """lfg_set_fused_motion_interpolate(1): the motion kernels write the generated frame as they decide each vector -- on three
    workgroups that each take many units, the bytes of motion-then-interpolate on a default context."""
    size, name = REPLAN_PAIR
    prev, curr, _ = gc.pairs_of(size)[name]
    p, q, a = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(*size)
    ctx.set_fused_motion_interpolate(False)
    want = {}
    for t in (0.5, 0.25):
        ctx.interpolate_frames(p, q, a, t)
        want[t] = ctx.download(a)
    for f in (p, q, a):
        ctx.destroy_frame(f)
    assert not (want[0.5] == want[0.25]).all()
    with knob_context(monkeypatch, dict(LFG_PREF_GROUPS="3")) as c:
        p, q, b = c.frame_from(prev), c.frame_from(curr), c.create_frame(*size)
        c.set_fused_motion_interpolate(True)
        for t in (0.5, 0.25, 0.5):
            c.upload(b, np.full((size[1], size[0], 4), 0xA5, np.uint8))         # (every pixel has to be written)
            c.interpolate_frames(p, q, b, t)
            got = c.download(b)
            assert (got == want[t]).all(), f"factor {t}: {first_bad(got, want[t])}"
