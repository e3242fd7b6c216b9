"""The route of lfg_interpolate_frames[_multi], stated once on the CPU side: which of the twelve context settings apply
together, and the CPU chain of the route that results.  Shared by tests/test_route_cases.py (CPU: the cases can fail),
tests/test_gpu_routes.py (GPU: the dispatch of lfg_capi.cpp against the chain) and tests/host_stream_cases.py (lfg_host's loop).

A ``Route`` is a setting of tests/cases.py -- (estimator, radius, interpolator, semantics) -- with the fused order, match_sad
and the seven later switches: cut detection, the generation mode, static protection, the bidirectional route, half-resolution
motion, the hole reach and quarter-pixel vectors.  ``cut`` is "off", "passes" (on, with the chain's threshold that the pair
passes), "fails" (on, with the one it fails), or a threshold 0 .. 1000 of the caller's own.

``effective(route)`` is written from include/linuxfg_hip.h (the paragraphs of the lfg_set_* calls) and DESIGN.md section 2,
not from the library's code: the route with every switch that the header says does not apply put back to off, the compensated
kind that runs and whether that kind fills its holes from the fill plane.  Two routes with equal effective() are defined to
give the same bytes on any input.

``RouteChain(prev, curr)`` composes the existing models -- nothing in it is a model of its own."""
from __future__ import annotations

import itertools
from collections import namedtuple

import numpy as np

from tests import bidir_model as bm
from tests import cases
from tests import expand_model as xm
from tests import extrapolate_model as ex
from tests import fill_model as fm
from tests import mc_model as mc
from tests import overlay_model as ov
from tests import pair_model as pair
from tests import pyramid_model as pm
from tests import refine_model as rm
from tests import subpel_model as sp

ROOM = 150                                          # pixels per thousand between a pair and either threshold (host_stream_cases.ROOM)
WALK = 16                                           # the hole walk's reach: lfg_set_hole_reach(16) is the walk, by definition

_FIELDS = ("estimator", "radius", "interpolator", "semantics", "fused", "match_sad", "cut", "generation", "protect", "bidirectional",
           "half_res", "reach", "subpel")
Route = namedtuple("Route", _FIELDS, defaults=(False, mc.DEFAULT_MATCH_SAD, "off", "interpolate", -1, -1, -1, -1, -1))
Effective = namedtuple("Effective", _FIELDS + ("kind", "fill"))
KINDS = ("shader", "plain", "masked", "extrapolate", "bidirectional", "subpel", "fallback", "newest")


def route(setting, **switches) -> Route:
    return Route(*setting, **switches)


def effective(r: Route) -> Effective:
    """The header's precedence, in its own order:
      a cut (lfg_set_cut_detection): every output is a source frame, whatever else is set -- curr for every output where
        extrapolation applies ("newest"), else prev below 0.5 and curr from there on ("fallback"); a pair that passes its
        threshold is presented as with detection off;
      the fused order changes no byte on any route;
      LFG_INTERPOLATOR_SHADER: generation, protection, bidirectional, reach and sub-pixel vectors are stored and have no effect;
        match_sad is the compensated kinds' and the record's alone; the estimator, the refinement, the semantics and
        half-resolution motion apply;
      LFG_INTERPOLATOR_COMPENSATED: the semantics reach the bytes through the full search only;
        LFG_GENERATION_EXTRAPOLATE beats everything: protection, bidirectional, reach and sub-pixel vectors have no effect;
        static protection switches bidirectional and sub-pixel vectors off and takes the reach (pass_static = 1);
        bidirectional switches sub-pixel vectors off and takes the reach;
        a reach switches sub-pixel vectors off -- at 16 too, where the plane is the walk and the bytes are the walk's;
        sub-pixel vectors apply where none of those is on;
      half-resolution motion and the refinement apply to every field that is measured, on every route."""
    assert r.cut in ("off", "passes", "fails"), f"resolve a numeric threshold first (RouteChain.resolved): {r.cut}"
    compensated = r.interpolator == "compensated"
    ahead = compensated and r.generation == "extrapolate"
    if r.cut == "fails":
        return Effective("full", -1, "shader", 0, False, mc.DEFAULT_MATCH_SAD, "fails", "extrapolate" if ahead else "interpolate", -1, -1, -1,
                         -1, -1, "newest" if ahead else "fallback", False)
    e = dict(r._asdict(), fused=False, cut="off")
    if not compensated:
        e.update(match_sad=mc.DEFAULT_MATCH_SAD, generation="interpolate", protect=-1, bidirectional=-1, reach=-1, subpel=-1)
        return Effective(**e, kind="shader", fill=False)
    if r.estimator == "pyramid":
        e.update(semantics=1)
    if ahead:
        e.update(protect=-1, bidirectional=-1, reach=-1, subpel=-1)
        return Effective(**e, kind="extrapolate", fill=False)
    fill = r.reach >= 1 and r.reach != WALK
    if r.reach == WALK:
        e.update(reach=-1)
    if r.protect >= 0:
        e.update(bidirectional=-1, subpel=-1)
        return Effective(**e, kind="masked", fill=fill)
    if r.bidirectional >= 0:
        e.update(subpel=-1)
        return Effective(**e, kind="bidirectional", fill=fill)
    if r.reach >= 1:
        e.update(subpel=-1)
        return Effective(**e, kind="plain", fill=fill)
    return Effective(**e, kind="subpel" if r.subpel >= 0 else "plain", fill=False)


def measures_backward(r: Route) -> bool:
    """Whether the route measures the pair the other way too (cut or not: the record is taken before the fallback)."""
    return r.interpolator == "compensated" and r.generation == "interpolate" and r.protect < 0 and r.bidirectional >= 0


class RouteChain(cases.Chain):
    """cases.Chain with the seven switches.  `passes` and `fails` are the thresholds of the cut states "passes" and "fails"
    (thresholds() derives them from the pair).  Everything is kept: vectors by what the field depends on, frames by
    effective(route) and factor, so 192 routes cost a few dozen model runs; what is returned is shared: compare, do not write."""

    def __init__(self, prev, curr, passes=None, fails=None):
        super().__init__(prev, curr)
        self.passes, self.fails = passes, fails
        self._reverse = cases.Chain(curr, prev)
        self._half, self._stats, self._by_route, self._masks, self._quarter = {}, {}, {}, {}, {}

    # ---- vectors

    def _field(self, r: Route, backward: bool):
        chain = self._reverse if backward else self
        if r.half_res < 0:
            return cases.Chain.vectors(chain, r.estimator, r.radius, r.semantics)
        k = (backward, r.estimator, r.semantics if r.estimator == "full" else None, r.half_res)
        if k not in self._half:
            a, b = chain.prev, chain.curr
            ha, hb = xm.halve(a), xm.halve(b)
            if r.estimator == "pyramid":
                low = pm.motion_pyramid(ha, hb, 1, 16, 2)
            else:
                import oracle
                low = oracle.motion(ha, hb, semantics=r.semantics).astype(np.int8)
            self._half[k] = xm.expand(a, b, low, r.half_res)
        if r.radius < 0:
            return self._half[k]
        if k + (r.radius,) not in self._half:
            self._half[k + (r.radius,)] = rm.refine(chain.prev, chain.curr, self._half[k], r.radius)
        return self._half[k + (r.radius,)]

    def vectors(self, r: Route):
        """(the final integer field, the same for the reversed pair where the bidirectional route applies, else None)."""
        return self._field(r, False), (self._field(r, True) if measures_backward(r) else None)

    # ---- the record and the verdict

    def stats(self, r: Route):
        """lfg_last_pair_stats' record: pair_model.pair_stats on the final integer forward field."""
        mv = self._field(r, False)
        k = (id(mv), r.match_sad)
        if k not in self._stats:
            self._stats[k] = pair.pair_stats(self.prev, self.curr, mv, r.match_sad)
        return self._stats[k]

    def threshold(self, r: Route) -> int:
        """What lfg_set_cut_detection is given for the route: -1 for off."""
        if r.cut == "off":
            return -1
        if r.cut in ("passes", "fails"):
            t = self.passes if r.cut == "passes" else self.fails
            assert t is not None, "this chain was made without thresholds"
            return t
        return int(r.cut)

    def is_cut(self, r: Route) -> bool:
        return r.cut != "off" and pair.cut(self.stats(r), self.threshold(r))

    def resolved(self, r: Route) -> Route:
        """The route with its cut state as the record decides it under the route's threshold."""
        return r._replace(cut="fails" if self.is_cut(r) else "off")

    # ---- frames

    def _generate(self, e: Effective, t: float):
        prev, curr, ms = self.prev, self.curr, e.match_sad
        if e.kind in ("fallback", "newest"):
            return curr if e.kind == "newest" else pair.fallback(prev, curr, [t])[0]
        r = Route(*e[:len(_FIELDS)])
        fwd, bwd = self.vectors(r)
        if e.kind == "shader":
            import oracle
            return oracle.interpolate(prev, curr, fwd.astype(np.float32), t, semantics=e.semantics)
        if e.kind == "extrapolate":
            return ex.extrapolate(prev, curr, fwd, t, ms)
        if e.kind == "subpel":
            k = (id(fwd), e.subpel)
            if k not in self._quarter:
                self._quarter[k] = sp.refine(prev, curr, fwd, e.subpel)
            return sp.interpolate(prev, curr, self._quarter[k], t, ms)
        if e.kind == "masked":
            if e.protect not in self._masks:
                self._masks[e.protect] = ov.static_mask(prev, curr, e.protect)
            mask = self._masks[e.protect]
            return fm.interpolate_masked(prev, curr, fwd, mask, t, e.reach, ms) if e.fill else ov.interpolate_masked(prev, curr, fwd, mask, t, ms)
        if e.kind == "bidirectional":
            if e.fill:
                return fm.interpolate_bidirectional(prev, curr, fwd, bwd, t, e.reach, ms, e.bidirectional)
            return bm.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, e.bidirectional)
        assert e.kind == "plain", e.kind
        return fm.interpolate_compensated(prev, curr, fwd, t, e.reach, ms) if e.fill else mc.interpolate_compensated(prev, curr, fwd, t, ms)

    def frames(self, r: Route, factors):
        """The frames that lfg_interpolate_frames[_multi] must give under the route, one per factor."""
        e = effective(self.resolved(r))
        out = []
        for t in factors:
            k = (e, float(t))
            if k not in self._by_route:
                self._by_route[k] = self._generate(e, float(t))
            out.append(self._by_route[k])
        return out


def thresholds(chain: RouteChain, routes):
    """(passes, fails): one threshold that every record of `routes` passes with ROOM to spare and one that every record fails
    by as much, from pair_model.permille of the pair under each route's field and match_sad."""
    p = [pair.permille(chain.stats(r)) for r in routes]
    passes, fails = min(p) - ROOM, max(p) + ROOM + 1              # permille() rounds down: + 1 keeps the room on the upper side
    assert 1 <= passes and fails <= 1000, f"the pair leaves no room: matched per thousand {min(p)} .. {max(p)}"
    return passes, fails


# ---- the scene

SCENE = (200, 120)
FAST = dict(size=40, at=(8, 4), shift=(48, 0))      # leaves a hole 40 px wide and high: its middle is out of the walk's reach
EDGES = ((24, (112, 8), (10, 6)), (28, (152, 50), (-14, 4)))
FRACTIONAL = dict(at=(8, 58), size=(48, 40), quarters=(10, -6))      # content that moves by (2.5, -1.5) px inside a window
NOISE = (slice(100, 118), slice(60, 196))           # uncorrelated in the two frames: what keeps the pair ROOM below 1000


def static_overlay(w, h):
    """(on, bytes, flicker): three one-pixel strokes and a block of noise that do not move, and `flicker`, a block whose bytes
    differ by 1 in two channels between the frames: static at tolerance 8, not at 0."""
    on = np.zeros((h, w), bool)
    px = np.zeros((h, w, 4), np.uint8)
    on[48, 20:140] = True
    on[10:96, 104] = True
    on[90, 60:190] = True
    px[on] = (255, 255, 255, 255)
    on[70:82, 112:128] = True
    px[70:82, 112:128] = np.random.default_rng(3).integers(0, 256, (12, 16, 4), dtype=np.uint8)
    flicker = np.zeros((h, w), bool)
    flicker[84:96, 150:190] = True
    return on, px, flicker


def route_scene():
    """(prev, curr) of 200 x 120 that tells the routes apart (test_route_cases.py: test_routes_that_differ_give_different_frames):
    a background panned by (4, -2); a square that moves 48 px and leaves a hole wider and higher than 32 px (reach 32 against
    the walk), whose revealed ground is an occlusion where the two fields disagree (bidirectional); two squares with motions of
    their own (moving edges: refinement, half resolution); a window whose content moves by (2.5, -1.5) px (sub-pixel); a static
    overlay of strokes and a noise block over all of it, with a part that flickers by 1 (protection 0 against 8); and a stripe
    of noise that is new in each frame, which no field explains."""
    from linux_fg_amd import synth
    w, h = SCENE
    seed = synth.BASE_SEED + 23
    bg = synth.make_prev(w, h, seed)
    prev, curr = bg.copy(), synth.translate(bg, (4, -2), seed)
    rng = np.random.default_rng(29)
    (fx, fy), (fw, fh) = FRACTIONAL["at"], FRACTIONAL["size"]
    from tests import subpel_cases
    a, b, _ = subpel_cases.fractional_pan(fw, fh, FRACTIONAL["quarters"], seed=31)
    prev[fy:fy + fh, fx:fx + fw], curr[fy:fy + fh, fx:fx + fw] = a, b
    for size, (x, y), (sx, sy) in ((FAST["size"], FAST["at"], FAST["shift"]),) + EDGES:
        tex = rng.integers(0, 256, (size, size, 4), dtype=np.uint8)
        prev[y:y + size, x:x + size] = tex
        curr[y + sy:y + sy + size, x + sx:x + sx + size] = tex
    prev[NOISE], curr[NOISE] = (rng.integers(0, 256, (18, 136, 4), dtype=np.uint8) for _ in range(2))
    on, px, flicker = static_overlay(w, h)
    still = rng.integers(8, 248, (h, w, 4), dtype=np.uint8)
    prev[flicker], curr[flicker] = still[flicker], still[flicker] + np.array([1, 0, 1, 0], np.uint8)
    prev[on], curr[on] = px[on], px[on]
    return prev, curr


# ---- the routes of the tests

BASE = ("pyramid", 1, "compensated", 1)
ON = dict(generation="extrapolate", protect=0, bidirectional=1, half_res=1, reach=32, subpel=1)
CUTS = ("off", "passes", "fails")


def matrix_routes():
    """All 3 x 2^6 combinations of the seven switches on BASE."""
    out = []
    for cut in CUTS:
        for on in itertools.product((False, True), repeat=len(ON)):
            out.append(route(BASE, cut=cut, **{k: v for (k, v), use in zip(ON.items(), on) if use}))
    return out


def route_id(r: Route) -> str:
    d = Route(*BASE)
    parts = ["-".join(str(v) for v in r[:4])] if tuple(r[:4]) != BASE else []
    parts += [f"{k}={getattr(r, k)}" for k in _FIELDS[4:] if getattr(r, k) != getattr(d, k)]
    return ",".join(parts) or "base"


SHADER = ("pyramid", 1, "shader", 1)
CROSS = (
    # the shader with each switch on in turn: only the cut and half resolution may change its bytes
    [route(SHADER)] + [route(SHADER, **{k: v}) for k, v in ON.items()] + [route(SHADER, cut="passes"), route(SHADER, cut="fails")] +
    # the fused order, which applies to neither
    [route(("full", -1, "shader", 0), fused=True, half_res=1), route(("full", -1, "shader", 0), fused=True, cut="passes"),
     route(("full", -1, "shader", 0), fused=True, cut="fails"), route(("full", -1, "shader", 0), fused=True)] +
    # the full search under the reference semantics, measured both ways on the halves, with the fill plane
    [route(("full", -1, "compensated", 0), bidirectional=1, half_res=1, reach=32),
     route(("full", 0, "compensated", 1), bidirectional=1, half_res=1, reach=32, cut="passes")] +
    # the refinement radii with both directions on the halves
    [route(("pyramid", -1, "compensated", 1), bidirectional=1, half_res=1), route(("pyramid", 2, "compensated", 1), bidirectional=1, half_res=1)] +
    # the other values of the switches
    [route(BASE, half_res=0), route(BASE, half_res=2), route(BASE, reach=16), route(BASE, reach=255), route(BASE, reach=16, subpel=1),
     route(BASE, subpel=0), route(BASE, subpel=2), route(BASE, protect=8), route(BASE, protect=8, reach=255), route(BASE, bidirectional=0),
     route(BASE, bidirectional=0, reach=16, half_res=2), route(BASE, match_sad=300, subpel=1), route(BASE, match_sad=100, cut="passes", reach=32)]
)


_scene_chain = None


def scene_chain() -> RouteChain:
    """The one RouteChain of route_scene() for a whole test session, with the thresholds of the matrix and the cross."""
    global _scene_chain
    if _scene_chain is None:
        chain = RouteChain(*route_scene())
        chain.passes, chain.fails = thresholds(chain, [r for r in matrix_routes() + CROSS if r.cut != "off"])
        _scene_chain = chain
    return _scene_chain
