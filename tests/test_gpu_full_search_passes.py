"""The per-pass loops of the persistent motion kernel's two full-search phases -- the narrow search (prefilter_narrow.inc) and the
row band (prefilter_rowband.inc) -- on what their bookkeeping decides and test_gpu_parity.py's interior strips do not isolate:
bands of every width class at every edge of the frame, lists that fill until the unit gives up, frames in flight, the variant
for moderate noise and the intended tie order.  448 x 320 frames: 8 x 5 prefilter tiles, rim and interior ones; the prefiltered
path against the literal kernel on the whole frame, byte for byte."""
import functools

import numpy as np
import pytest

from linux_fg_amd import synth
from tests.gpu_kit import ctx, three_lanes
from tests.test_gpu_parity import intended, run_motion_mode

pytestmark = pytest.mark.gpu

W, H = 448, 320
SEED = 9600


@functools.lru_cache(maxsize=None)
def pan(dx, dy):
    """A pan by (dx, dy): it exposes |dx| columns at one vertical edge and |dy| rows at one horizontal edge, filled with noise."""
    prev = synth.make_prev(W, H, seed=SEED)
    curr = synth.translate(prev, (dx, dy), SEED)
    for a in (prev, curr):
        a.setflags(write=False)
    return prev, curr


_literal = {}


def literal(ctx, dx, dy):
    """The literal kernel's vectors for pan(dx, dy) under the reference semantics: computed once, shared, left unchanged."""
    from linux_fg_amd import capi
    if (dx, dy) not in _literal:
        _literal[dx, dy], _ = run_motion_mode(ctx, *pan(dx, dy), capi.MOTION_EXACT_ONLY)
        _literal[dx, dy].setflags(write=False)
    return _literal[dx, dy]


@pytest.mark.parametrize("dy", [3, -3])
@pytest.mark.parametrize("dx", [2, -2, 6, -6, 10, -10])
def test_pans_expose_a_band_of_each_width_class_at_each_edge(ctx, dx, dy):
    """|dx| = 2, 6, 10: the pixels without a match are a band of 6, 10 and 14 columns -- 4, 3 and 2 candidates per pass of the
    narrow search -- at the left edge (dx > 0) or the right one; |dy| = 3: a band of 7 rows at the top (dy > 0) or the bottom.
    No tile may need the literal kernel."""
    from linux_fg_amd import capi
    got, st = run_motion_mode(ctx, *pan(dx, dy), capi.MOTION_PREFILTERED)
    want = literal(ctx, dx, dy)
    print(f"pan ({dx}, {dy}): {int((got != want).any(-1).sum())} pixels differ, {st[1]} tiles through the literal kernel")
    assert (got == want).all()
    assert st[1] == 0


def flat_strip(where):
    """A static pair whose rim is one colour in both frames, with a strip of ANOTHER colour along the edge of curr: ten columns at
    the left edge or six rows at the bottom.  The strip's pixels cost 8 x 8 x sqrt(4 x 40^2) = 5,120 with EVERY candidate whose
    block stays inside the flat rim of prev -- above the 2,048 of a pixel without a match, so they are searched in full as a
    narrow band (left) or a row band (bottom), hundreds of candidates tie, the lists fill and the unit gives up."""
    prev = synth.make_prev(W, H, seed=SEED + 1)
    if where == "left":
        prev[:, :30] = 140
        curr = prev.copy()
        curr[:, :10] = 100
    else:
        prev[H - 26:] = 140
        curr = prev.copy()
        curr[H - 6:] = 100
    return prev, curr


@pytest.mark.parametrize("where", ["left", "bottom"])
def test_a_flat_strip_fills_the_lists_and_the_unit_gives_up(ctx, where):
    from linux_fg_amd import capi
    prev, curr = flat_strip(where)
    got, st = run_motion_mode(ctx, prev, curr, capi.MOTION_PREFILTERED)
    want, _ = run_motion_mode(ctx, prev, curr, capi.MOTION_EXACT_ONLY)
    print(f"flat strip, {where}: {int((got != want).any(-1).sum())} pixels differ, {st[1]} tiles through the literal kernel")
    assert (got == want).all()
    assert st[1] > 0


def test_a_pan_with_three_frames_in_flight(ctx):
    """pan(6, -3) on each of three lanes, all enqueued before the one synchronisation."""
    from linux_fg_amd import capi
    prev, curr = pan(6, -3)
    want = literal(ctx, 6, -3)

    def enqueue(i, p, c):
        fp, fc = ctx.frame_from(p), ctx.frame_from(c)
        mv = ctx.create_frame(W, H, capi.FORMAT_MV_S8X2)
        ctx.motion(fp, fc, mv)
        return fp, fc, mv

    three_lanes(ctx, [(prev, curr)] * 3, enqueue, [want] * 3)


def test_a_pan_through_the_variant_for_moderate_noise(ctx, monkeypatch):
    """motion_prefilter_kernel<false, 1>, forced for every call of a context created under LFG_TIER_FORCE=1: the same includes,
    compiled a second time."""
    from linux_fg_amd import capi
    want = literal(ctx, 6, -3)
    monkeypatch.setenv("LFG_TIER_FORCE", "1")
    with capi.Context(0) as forced:
        got, st = run_motion_mode(forced, *pan(6, -3), capi.MOTION_PREFILTERED)
        assert forced.motion_last_variant() == 1
    assert (got == want).all()
    assert st[1] == 0


def test_a_pan_under_the_intended_tie_order(intended):
    from linux_fg_amd import capi
    got, st = run_motion_mode(intended, *pan(6, -3), capi.MOTION_PREFILTERED)
    want, _ = run_motion_mode(intended, *pan(6, -3), capi.MOTION_EXACT_ONLY)
    assert (got == want).all()
    assert st[1] == 0
