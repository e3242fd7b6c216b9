"""The cases of tests/route_cases.py can fail: on its scene any two routes that the header defines differently give different
frames, routes that it defines alike share their frames, the cut states fall where they are meant to with room to spare, and
the chain is the per-feature models' own word where the two overlap.  CPU only: the models of tests/ and the oracle."""
import itertools

import numpy as np
import pytest

from tests import bidir_cases as bc
from tests import bidir_model as bm
from tests import cases
from tests import expand_model as xm
from tests import extrapolate_model as ex
from tests import fill_cases as fc
from tests import fill_model as fm
from tests import overlay_model as ov
from tests import pair_model as pair
from tests import pyramid_model as pm
from tests import refine_model as rm
from tests import route_cases as rc
from tests import subpel_model as sp

FACTORS = [cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS
ROUTES = rc.matrix_routes() + rc.CROSS


@pytest.fixture(scope="module")
def chain(oracle):
    return rc.scene_chain()


def test_the_lists_are_what_the_tests_say_they_are():
    matrix = rc.matrix_routes()
    assert len(matrix) == len(set(matrix)) == 192 and all(tuple(r[:4]) == rc.BASE and not r.fused for r in matrix)
    assert {(r.generation, r.protect, r.bidirectional, r.half_res, r.reach, r.subpel) for r in matrix} == \
           set(itertools.product(("interpolate", "extrapolate"), (-1, 0), (-1, 1), (-1, 1), (-1, 32), (-1, 1)))
    assert len(rc.CROSS) == len(set(rc.CROSS)) >= 24 and not set(rc.CROSS) & set(matrix)
    cross = set(rc.CROSS)
    for k, v in rc.ON.items():
        assert rc.route(rc.SHADER, **{k: v}) in cross
    assert {r.half_res for r in cross} >= {0, 1, 2} and {r.reach for r in cross} >= {16, 32, 255}
    assert {r.subpel for r in cross} >= {0, 1, 2} and {r.protect for r in cross} >= {0, 8} and {r.bidirectional for r in cross} >= {0, 1}
    assert {r.radius for r in cross if r.bidirectional >= 0 and r.half_res >= 0} >= {-1, 2}
    assert any(r.fused and r.half_res >= 0 for r in cross) and any(r.fused and r.cut != "off" for r in cross)
    assert any(r.estimator == "full" and r.semantics == 0 and r.bidirectional >= 0 and r.half_res >= 0 and r.reach >= 1 for r in cross)


def test_the_precedence_is_the_headers():
    """effective() on combinations stated here by hand, one per sentence of the header."""
    def eff(**switches):
        e = rc.effective(rc.route(rc.BASE, **switches))
        return e.kind, e.fill, {k: getattr(e, k) for k in rc.ON if getattr(e, k) != getattr(rc.Route(*rc.BASE), k)}

    everything = dict(rc.ON)
    assert eff() == ("plain", False, {})
    assert eff(**everything) == ("extrapolate", False, dict(generation="extrapolate", half_res=1))       # extrapolation beats everything
    del everything["generation"]
    assert eff(**everything) == ("masked", True, dict(protect=0, half_res=1, reach=32))                   # protection switches both off
    del everything["protect"]
    assert eff(**everything) == ("bidirectional", True, dict(bidirectional=1, half_res=1, reach=32))      # bidirectional beats sub-pixel
    del everything["bidirectional"]
    assert eff(**everything) == ("plain", True, dict(half_res=1, reach=32))                               # and so does a reach
    del everything["reach"]
    assert eff(**everything) == ("subpel", False, dict(half_res=1, subpel=1))
    assert eff(reach=16, subpel=1) == ("plain", False, {})                                                # at 16 too: the walk's bytes
    assert eff(generation="extrapolate", reach=32) == ("extrapolate", False, dict(generation="extrapolate"))
    assert eff(cut="passes", reach=32) == eff(reach=32)
    assert eff(cut="fails", **rc.ON)[0] == "newest" and eff(cut="fails", protect=0, reach=32, half_res=1) == ("fallback", False, {})
    shader = rc.effective(rc.route(rc.SHADER, fused=True, match_sad=7, **{k: v for k, v in rc.ON.items() if k != "half_res"}))
    assert shader == rc.effective(rc.route(rc.SHADER)) and shader.kind == "shader"
    assert rc.effective(rc.route(rc.SHADER, half_res=1)) != shader
    assert rc.effective(rc.route(rc.SHADER, cut="fails", generation="extrapolate")).kind == "fallback"    # stored, no effect
    assert rc.effective(rc.route(("pyramid", 1, "compensated", 0))) == rc.effective(rc.route(rc.BASE))
    assert rc.effective(rc.route(("full", 1, "compensated", 0))) != rc.effective(rc.route(("full", 1, "compensated", 1)))
    # the matrix: six kinds with and without the halves, three of them with and without the plane, and the two fallbacks
    assert len({rc.effective(r) for r in rc.matrix_routes()}) == 2 * (2 + 2 + 1 + 1 + 1 + 1) + 2


def test_the_scene_leaves_room_on_both_sides_of_both_thresholds(chain):
    w, h = rc.SCENE
    assert chain.prev.shape == chain.curr.shape == (h, w, 4) and w <= 200 and h <= 120
    assert 1 <= chain.passes < chain.fails <= 1000
    for r in ROUTES:
        if r.cut == "off":
            continue
        p = pair.permille(chain.stats(r))
        assert chain.passes + rc.ROOM <= p <= chain.fails - rc.ROOM, (rc.route_id(r), p)
        assert chain.is_cut(r) == (r.cut == "fails")
        assert chain.threshold(r) == (chain.passes if r.cut == "passes" else chain.fails)
    print(f"matched per thousand {sorted({pair.permille(chain.stats(r)) for r in ROUTES if r.cut != 'off'})}, thresholds "
          f"{chain.passes} / {chain.fails}")


def test_the_scene_holds_what_the_routes_need(chain):
    """Each feature of the scene's docstring, shown on the chain's own fields."""
    base = rc.route(rc.BASE)
    fwd, _ = chain.vectors(base)
    # a hole wider than the walk reaches: some hole of K at t = 0.5 has no donor within 16 px and one within 32
    from tests import mc_model as mc
    K = mc.keys(chain.prev, chain.curr, fwd, 0.5)
    near, far = fm.plane(K, 16), fm.plane(K, 32)
    assert ((K == fm.HOLE) & (near == fm.HOLE) & (far != fm.HOLE)).sum() >= 16
    # an occlusion: the two fields disagree beyond the tolerance where the fast square uncovers the ground
    both = rc.route(rc.BASE, bidirectional=1)
    f, b = chain.vectors(both)
    assert (bm.consistency(f, b, 1) == 0).sum() >= 400
    # a static overlay, and a part of it that is static at tolerance 8 alone
    on, _, flicker = rc.static_overlay(*rc.SCENE)
    assert ov.static_mask(chain.prev, chain.curr, 0)[on].all() and not ov.static_mask(chain.prev, chain.curr, 0)[flicker & ~on].any()
    assert ov.static_mask(chain.prev, chain.curr, 8)[flicker & ~on].all()
    # fractional motion: the quarter-pixel refinement leaves the integer grid on most of the window
    (x, y), (w, h) = rc.FRACTIONAL["at"], rc.FRACTIONAL["size"]
    q = sp.refine(chain.prev, chain.curr, fwd, 1)[y + 8:y + h - 8, x + 8:x + w - 8]
    assert ((q % 4) != 0).any(-1).mean() > 0.5
    # moving edges: the refinement and the halves both change the field
    assert (fwd != chain.vectors(base._replace(radius=-1))[0]).any() and (fwd != chain.vectors(base._replace(half_res=1))[0]).any()


def test_routes_that_differ_give_different_frames(chain):
    """A condition, not a measurement: any two routes of the matrix and the cross whose effective() differ give different bytes
    at at least one factor, so a dispatch that runs a neighbour's route fails the GPU matrix.  No pair is exempt."""
    by = {}
    for r in ROUTES:
        by.setdefault(rc.effective(chain.resolved(r)), chain.frames(r, FACTORS))
    fewest = None
    for (a, fa), (b, fb) in itertools.combinations(by.items(), 2):
        differing = max(int((x != y).any(-1).sum()) for x, y in zip(fa, fb))
        assert differing > 0, f"the scene cannot tell\n{a}\nfrom\n{b}"
        fewest = differing if fewest is None else min(fewest, differing)
    print(f"{len(ROUTES)} routes, {len(by)} effective ones, the closest two differ on {fewest} pixels of their most different frame")
    assert len(by) >= 36


def test_routes_that_are_defined_alike_share_their_frames(chain):
    """Equal effective(): the very same arrays -- the memoisation works and an ignored switch is ignored."""
    first = {}
    shared = 0
    for r in ROUTES:
        e = rc.effective(chain.resolved(r))
        frames = chain.frames(r, FACTORS)
        if e in first:
            assert all(x is y for x, y in zip(frames, first[e])), rc.route_id(r)
            shared += 1
        first.setdefault(e, frames)
    assert shared >= 150


def test_a_cut_presents_the_fallback_and_a_pass_the_generated_frames(chain):
    prev, curr = chain.prev, chain.curr
    for r in ROUTES:
        if r.cut == "off":
            continue
        frames = chain.frames(r, FACTORS)
        ahead = r.interpolator == "compensated" and r.generation == "extrapolate"
        if r.cut == "fails":
            want = [curr] * len(FACTORS) if ahead else pair.fallback(prev, curr, FACTORS)
            assert all(f is e for f, e in zip(frames, want)), rc.route_id(r)
        else:
            off = chain.frames(r._replace(cut="off"), FACTORS)
            assert all(f is e for f, e in zip(frames, off)), rc.route_id(r)
            assert not any(f is prev or f is curr or (f == curr).all() or (f == prev).all() for f in frames), rc.route_id(r)
    assert [f is curr for f in pair.fallback(prev, curr, FACTORS)] == [False, False, True, True, True]      # both sources are shown


# ---- the chain is no second opinion: against the per-feature models and case files where they overlap

def planted(prev, curr, fwd, bwd=None):
    """A RouteChain whose pyramid has already "measured" fwd and, the other way, bwd."""
    chain = rc.RouteChain(prev, curr)
    chain._estimated[("pyramid", None)] = fwd
    if bwd is not None:
        chain._reverse._estimated[("pyramid", None)] = bwd
    return chain


RAW = ("pyramid", -1, "compensated", 1)


def test_chain_is_the_fill_cases_scene_b_at_reach_32():
    (prev, _, curr), fwd, bwd = fc.scene_fields(fm.SCENE_B)
    chain = planted(prev, curr, fwd, bwd)
    mask = ov.static_mask(prev, curr, 0)
    for t in (0.5, 0.3):
        assert (chain.frames(rc.route(RAW, reach=32), [t])[0] == fm.interpolate_compensated(prev, curr, fwd, t, 32, 48)).all()
        assert (chain.frames(rc.route(RAW, reach=32, protect=0, bidirectional=1, subpel=1), [t])[0] ==
                fm.interpolate_masked(prev, curr, fwd, mask, t, 32, 48)).all()
        assert (chain.frames(rc.route(RAW, reach=32, bidirectional=1, subpel=1), [t])[0] ==
                fm.interpolate_bidirectional(prev, curr, fwd, bwd, t, 32, 48, 1)).all()
        walk = chain.frames(rc.route(RAW), [t])[0]
        assert chain.frames(rc.route(RAW, reach=16), [t])[0] is walk
        assert (walk == fm.interpolate_compensated(prev, curr, fwd, t, 16, 48)).all()
        assert (walk != chain.frames(rc.route(RAW, reach=32), [t])[0]).any()


@pytest.mark.parametrize("kind", ["piecewise", "small"])
def test_chain_is_the_bidir_cases(kind):
    prev, curr, fwd, bwd = bc.field(kind, 64, 48, 5)
    chain = planted(prev, curr, fwd, bwd)
    for tolerance, ms, t in ((0, 48, 0.3), (1, 1020, 0.5), (64, 48, 0.9)):
        got = chain.frames(rc.route(RAW, bidirectional=tolerance, match_sad=ms), [t])[0]
        assert (got == bm.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tolerance)).all(), (tolerance, ms, t)
    assert (chain.frames(rc.route(RAW, generation="extrapolate", bidirectional=1, reach=32), [0.7])[0] == ex.extrapolate(prev, curr, fwd, 0.7, 48)).all()
    assert (chain.frames(rc.route(RAW, subpel=1), [0.7])[0] == sp.interpolate(prev, curr, sp.refine(prev, curr, fwd, 1), 0.7, 48)).all()
    assert chain.stats(rc.route(RAW, cut=500, match_sad=100)) == pair.pair_stats(prev, curr, fwd, 100)


def test_chain_vectors_are_the_models_in_the_headers_order(oracle):
    """Half resolution: the halves, the estimator's model on them (the pyramid at 1, 16, 2), the expansion, then the
    refinement -- and the same on the reversed pair."""
    prev, curr = cases.small_scene(64, 36, 71)
    chain = rc.RouteChain(prev, curr)
    for a, b, which in ((prev, curr, 0), (curr, prev, 1)):
        ha, hb = xm.halve(a), xm.halve(b)
        want = rm.refine(a, b, xm.expand(a, b, pm.motion_pyramid(ha, hb, 1, 16, 2), 2), 1)
        assert (chain.vectors(rc.route(rc.BASE, half_res=2, bidirectional=1))[which] == want).all()
        low = oracle.motion(ha, hb, semantics=0).astype(np.int8)
        assert (chain.vectors(rc.route(("full", -1, "compensated", 0), half_res=0, bidirectional=0))[which] == xm.expand(a, b, low, 0)).all()
    assert chain.vectors(rc.route(rc.BASE, half_res=2, bidirectional=1, protect=0))[1] is None
    assert chain.vectors(rc.route(rc.BASE, bidirectional=1, generation="extrapolate"))[1] is None
    assert (chain.vectors(rc.route(rc.BASE))[0] == cases.Chain(prev, curr).vectors("pyramid", 1, 1)).all()
