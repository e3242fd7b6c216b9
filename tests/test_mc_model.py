"""Known answers for the CPU model of lfg_interpolate_compensated (tests/mc_model.py): t = 1, an even pan, one hand-worked
8 x 8 case per rule of the header's definition, and the moving square that the shader's intended mode gets wrong.  And the
power of two sets that the GPU tests rely on (tests/cases.py): the inexact factors against the model's mutants, and the scene of
the dispatch matrix against the settings."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import cases
from tests import mc_model as mc

HOLE, key = mc.HOLE, mc.key


def unorm_pack(v: np.ndarray) -> np.ndarray:
    """float32 in 0..1 -> bytes as the library stores them."""
    return np.rint(np.clip(v.astype(np.float32) * np.float32(255.0), 0, 255)).astype(np.uint8)


def unorm(b) -> np.ndarray:
    return np.asarray(b, np.uint8).astype(np.float32) / np.float32(255.0)


def mix(p, c, t):
    t = np.float32(t)
    return unorm(p) * (np.float32(1.0) - t) + unorm(c) * t


textured = cases.textured


def test_unorm_round_trip_is_exact():
    k = np.arange(256, dtype=np.uint8)
    assert (unorm_pack(unorm(k)) == k).all()


@pytest.mark.parametrize("match_sad", [0, 48, 1020])
def test_t1_gives_curr_on_random_fields(match_sad):
    for w, h, seed in ((1, 1, 1), (7, 5, 2), (50, 40, 3)):
        prev, curr = textured(w, h, seed), textured(w, h, seed + 100)
        mv = np.random.default_rng(seed).integers(-128, 128, (h, w, 2)).astype(np.int8)
        assert (mc.interpolate_compensated(prev, curr, mv, 1.0, match_sad) == curr).all()


def test_even_pan_at_half_is_exact_on_the_interior():
    prev = synth.make_prev(96, 64)
    curr = synth.translate(prev, (6, -4))
    mv = np.zeros((64, 96, 2), np.int8)
    mv[...] = (-6, 4)
    got = mc.interpolate_compensated(prev, curr, mv, 0.5)
    want = synth.translate(prev, (3, -2))
    assert (got[8:-8, 8:-8] == want[8:-8, 8:-8]).all()


def test_pan_with_estimated_vectors():
    """The shader's full search (oracle, intended tie order) on the same pan: exact 16 px from the border; sources in the
    unmatched strip can match by chance and project at most 6 + 8 px inwards."""
    import oracle as o
    o.build()
    prev = synth.make_prev(96, 64)
    curr = synth.translate(prev, (6, -4))
    mv = o.motion(prev, curr, semantics=o.INTENDED).astype(np.int8)
    got = mc.interpolate_compensated(prev, curr, mv, 0.5)
    want = synth.translate(prev, (3, -2))
    assert (got[16:-16, 16:-16] == want[16:-16, 16:-16]).all()


# ---- hand-worked 8 x 8 cases.  At t = 0.5 a vector v projects by floor(v * 0.5 + 0.5), i.e. v / 2 for even v.

# The inputs that need no hand-placed key image are built in tests/cases.py: test_gpu_compensated.py runs them on the GPU.

def test_collision_longest_then_vy_then_vx():
    prev, curr, mv, winners = cases.mc_collision()
    assert winners == {(4, 4): (-4, 0), (4, 3): (0, -2), (3, 6): (-2, 0)}
    K = mc.keys(prev, curr, mv, 0.5, 0)
    assert K[4, 4] == key(-4, 0)
    assert K[3, 4] == key(0, -2)
    assert K[6, 3] == key(-2, 0)
    prev, curr, mv, _ = cases.mc_collision(textured_frames=True)       # the same keys where every pixel matches by the gate
    assert (mc.keys(prev, curr, mv, 0.5, 1020) == K).all()


def test_unmatched_source_does_not_project():
    prev, curr, mv = cases.mc_unmatched_source()         # curr(3, 3) against prev(5, 3): SAD 200; (2, 0) -> (4, 3)
    K = mc.keys(prev, curr, mv, 0.5, 199)
    assert K[3, 4] == key(0, 0) and K[3, 3] == HOLE
    K = mc.keys(prev, curr, mv, 0.5, 200)
    assert K[3, 4] == key(2, 0) and K[3, 3] == HOLE


def test_projection_outside_the_image_is_dropped():
    prev, curr, mv = cases.mc_projection_outside()       # (0, 0) -> (0, -1), (7, 7) -> (9, 7)
    K = mc.keys(prev, curr, mv, 0.5, 0)
    assert K[0, 0] == HOLE and K[7, 7] == HOLE
    assert (K == HOLE).sum() == 2 and (K[K != HOLE] == key(0, 0)).all()


# The sampling step from hand-made key images.  With textured frames, match_sad 1020 (every pixel matches) and the vector u
# everywhere in mv, a hole filled with u is sampled exactly as a pixel that holds key(u).

def textured_case(u, w=16, h=16):
    prev, curr = textured(w, h, 41), textured(w, h, 42)
    mv = np.zeros((h, w, 2), np.int8)
    mv[...] = u
    return prev, curr, mv


def test_hole_fill_takes_the_smallest_vector_of_the_four_directions():
    K = np.full((16, 16), key(0, 0), np.uint32)
    K[8, 8] = HOLE
    K[8, 9] = key(3, 0)                                  # right, |v|^2 9
    K[8, 7] = HOLE; K[8, 6] = key(0, 2)                  # left: the first non-hole, |v|^2 4
    K[9, 8] = key(-1, 1)                                 # down, |v|^2 2
    K[7, 8] = key(1, -1)                                 # up, |v|^2 2 and the smaller vy: the fill vector
    prev, curr, mv = textured_case((1, -1))
    got = mc.sample(prev, curr, mv, K, 0.5, 1020)[8, 8]
    for u, same in (((1, -1), True), ((-1, 1), False), ((0, 2), False), ((3, 0), False)):
        K2 = K.copy()
        K2[8, 8] = key(*u)
        assert (mc.sample(prev, curr, mv, K2, 0.5, 1020)[8, 8] == got).all() == same, u


def test_hole_with_nothing_within_16_gets_zero():
    K = np.full((40, 40), HOLE, np.uint32)
    K[20, 37] = key(5, 0)                                # 17 to the right of (20, 20): out of reach
    prev, curr, mv = textured_case((0, 0), 40, 40)
    for t in (0.25, 0.5):
        got = mc.sample(prev, curr, mv, K, t, 1020)
        assert (got[20, 20] == unorm_pack(mix(prev[20, 20], curr[20, 20], t))).all()    # u = (0,0): both samples at the centre
    assert (mc.sample(prev, curr, mv, np.full((40, 40), HOLE, np.uint32), 0.5, 1020)
            == unorm_pack(mix(prev, curr, 0.5))).all()


def test_the_walk_reaches_16_through_the_call():
    """cases.mc_walk_reach: the one projected pixel, (20, 20), changes exactly the holes that find it within 16 steps."""
    prev, curr, mv, blank = cases.mc_walk_reach()
    for t in cases.WALK_REACH_FACTORS:
        K = mc.keys(prev, curr, mv, t, cases.WALK_REACH_MATCH_SAD)
        assert K[20, 20] == key(2, 0) and (K != HOLE).sum() == 1, t
        assert (mc.keys(prev, curr, blank, t, cases.WALK_REACH_MATCH_SAD) == HOLE).all(), t
        cases.check_walk_reach(mc.interpolate_compensated(prev, curr, mv, t, cases.WALK_REACH_MATCH_SAD),
                               mc.interpolate_compensated(prev, curr, blank, t, cases.WALK_REACH_MATCH_SAD), t)


def test_revealed_content_comes_from_curr_and_covered_from_prev():
    prev, curr, mv, obj = cases.mc_revealed_and_covered()    # an object moves from (4, 2) to (6, 2): v(6, 2) = (-2, 0)
    K = mc.keys(prev, curr, mv, 0.5, 0)
    # (4, 2) is unmatched (curr 0 against prev obj) and (6, 2) moved away: two holes; the object lands on (5, 2)
    assert K[2, 5] == key(-2, 0) and K[2, 4] == HOLE and K[2, 6] == HOLE
    out = mc.interpolate_compensated(prev, curr, mv, 0.5, 0)
    assert (out[2, 5] == obj).all()                      # half way
    # hole (4, 2): fill (0, 0), c = (4, 2) unmatched -> revealed, curr alone (black)
    assert (out[2, 4] == curr[2, 4]).all()
    # hole (6, 2): fill (0, 0), c = (6, 2) matched with (-2, 0) != (0, 0) -> covered, prev alone (black)
    assert (out[2, 6] == prev[2, 6]).all()
    # the same with textured frames, where the two rules give different bytes
    prev, curr = textured(8, 8, 51), textured(8, 8, 52)
    mv = np.zeros((8, 8, 2), np.int8)
    K = np.full((8, 8), key(0, 0), np.uint32)
    K[2, 4] = HOLE
    out = mc.sample(prev, curr, mv, K, 0.5, 0)           # c = (4, 2) unmatched (random content) -> curr
    assert (out[2, 4] == curr[2, 4]).all()
    mv[2, 4] = (1, 0)
    out = mc.sample(prev, curr, mv, K, 0.5, 1020)        # c matched with (1, 0) != (0, 0) -> prev
    assert (out[2, 4] == prev[2, 4]).all()


def test_one_sample_inside_and_one_outside():
    prev, curr, mv = textured_case((0, 0), 8, 8)
    K = np.full((8, 8), key(0, 0), np.uint32)
    wants = {
        (4, 0): prev[1, 3],                              # P = 1.5 + 2 = 3.5 inside, C = 1.5 - 2 < 0 outside: prev alone
        (-4, 0): curr[1, 3],                             # P = -0.5 outside, C = 3.5 inside: curr alone
        (4, -4): unorm_pack(mix(prev[0, 3], curr[3, 0], 0.5)),   # both outside: the blend of the clamped samples
    }
    for u, want in wants.items():
        K2 = K.copy()
        K2[1, 1] = key(*u)
        assert (mc.sample(prev, curr, mv, K2, 0.5, 1020)[1, 1] == want).all(), u
    # and through the projection: row 3 moves up by 4 and lands on row 1, whose prev sample (y = -0.5) is outside
    prev, curr, mv = cases.mc_row_projected_to_the_top()
    assert (mc.keys(prev, curr, mv, 0.5, 1020)[1] == key(0, -4)).all()
    assert (mc.interpolate_compensated(prev, curr, mv, 0.5, 1020)[1] == curr[3]).all()


def test_moving_square_is_exact_where_the_definition_is():
    prev, curr, (x, y) = mc.moving_square()
    import oracle as o
    o.build()
    mv = o.motion(prev, curr, semantics=o.INTENDED).astype(np.int8)
    bg = np.random.default_rng(7).integers(0, 256, prev.shape, dtype=np.uint8)     # moving_square's own background
    for t in (0.25, 0.5, 0.75):
        s = int(12 * t)
        truth = bg.copy()
        truth[y:y + 16, x + s:x + s + 16] = prev[y:y + 16, x:x + 16]
        got = mc.interpolate_compensated(prev, curr, mv, t)
        ok = (got == truth).all(-1)
        assert ok[y + 4:y + 12, x + s + 4:x + s + 12].all(), t                       # the square's interior
        swept = np.zeros_like(ok)
        swept[y - 4:y + 20, x - 4:x + 12 + 20] = True
        assert ok[~swept].all(), t                                                  # background >= 4 px outside the sweep
        # intended mode of the shader's interpolation: a double image on the square
        ref = o.interpolate(prev, curr, mv.astype(np.float32), t, semantics=o.INTENDED)
        assert (ref[y + 4:y + 12, x + s + 4:x + s + 12] == truth[y + 4:y + 12, x + s + 4:x + s + 12]).all(-1).mean() < 0.05, t


def test_roi_equals_the_whole_frame():
    prev, curr = textured(70, 50, 31), textured(70, 50, 32)
    mv = np.random.default_rng(3).integers(-20, 21, (50, 70, 2)).astype(np.int8)
    whole = mc.interpolate_compensated(prev, curr, mv, 0.3, 400)
    for x, y, w, h in ((0, 0, 70, 50), (5, 7, 20, 11), (60, 40, 10, 10)):
        assert (mc.interpolate_compensated(prev, curr, mv, 0.3, 400, roi=(x, y, w, h)) == whole[y:y + h, x:x + w]).all()


# ---- the power of what the GPU tests rely on

@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_inexact_factors_tell_the_mutants_from_the_model(mutant):
    """Three rewrites of the position arithmetic that are exact in real numbers (tests/mc_model.c): the curr position as
    P - u, the projection as v - ceil(v t - 0.5), the curr position with its half pixel added last.  On the dense random
    field of test_gpu_compensated.py at 257 x 131 each gives the model's bytes at every dyadic factor -- the products are exact
    there, which is why the GPU tests were blind to such a rewrite while they ran those alone -- and different bytes at
    inexact factors that the GPU tests now run (cases.INEXACT_FACTORS).  Pixels that differ at match_sad 1020:
        t             0.3    0.7    0.9    5/6
        C_FROM_P      172    390    546    714
        CEIL_PROJECT  2340   2472   6172   9049
        HALF_LAST     0      0      3      6
    The third is why 0.9 and 5/6 are in the set and why the frame is this large: it shows on a few pixels only.  Each mutant
    must show at two factors or more, so the set survives the loss of one."""
    prev, curr, mv = cases.field("random", 257, 131, 57)
    for t in cases.DYADIC_FACTORS:
        assert (mc.interpolate_compensated(prev, curr, mv, t, 1020, mutant=mutant)
                == mc.interpolate_compensated(prev, curr, mv, t, 1020)).all(), t
    differ = {t: int((mc.interpolate_compensated(prev, curr, mv, t, 1020, mutant=mutant)
                      != mc.interpolate_compensated(prev, curr, mv, t, 1020)).any(-1).sum()) for t in cases.INEXACT_FACTORS}
    print(mutant, differ)
    assert sum(n > 0 for n in differ.values()) >= 2, differ


def test_matrix_scene_tells_the_settings_apart():
    """The scene and the factors of the dispatch matrix (test_gpu_dispatch.py): any two settings that the header defines
    differently give different frames in the CPU chain, so a mixed-up branch cannot hide.  The only coincidences are the ones
    the header demands: pyramid + compensated depends on neither semantics (28 distinct frames of 32)."""
    prev, curr = cases.matrix_scene()
    ch = cases.Chain(prev, curr)
    factors = [cases.MATRIX_FACTOR] + cases.MATRIX_FACTORS
    frames = {s: ch.frames(s, factors) for s in cases.SETTINGS}
    for k, t in enumerate(factors):
        for i, a in enumerate(cases.SETTINGS):
            for b in cases.SETTINGS[i + 1:]:
                same = (frames[a][k] == frames[b][k]).all()
                assert same == cases.same_by_definition(a, b), (t, a, b)
        assert len({frames[s][k].tobytes() for s in cases.SETTINGS}) == 28, t
