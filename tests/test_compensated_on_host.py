"""The compensated family's kernels run on the CPU (tests/cpp/compensated_on_host.cpp over tests/cpp/hip_on_host): the .hip files
compiled by g++ as they are, their own launch_* functions, every frame, vector field and mask its own allocation that ends where
its last row ends -- tight, with ASan-poisoned row padding, and with a pitch that is only as aligned as the call asks for -- and
every output byte held to the model its GPU test holds it to.  The GPU tests see a wrong byte; only this sees a byte read or
written outside a frame that a gate or a weight of 0 then discards.  Built plainly and with -fsanitize=address,undefined (the
fill plane's driver also with -fsanitize=thread); the sanitized code is always the stand-alone program.  CPU only."""
import numpy as np
import pytest

from tests import bicubic_cases, bicubic_model, bidir_cases, bidir_model, cases, extrapolate_cases, extrapolate_model, fill_cases
from tests import fill_model, mc_model, on_host_kit as kit, overlay_cases, overlay_model, subpel_cases, subpel_model
from tests.on_host_kit import end_fields, end_fields_q, f32, sweep

HIP = ["interpolate_mc.hip", "extrapolate_mc.hip", "interpolate_bidir.hip", "interpolate_subpel.hip", "static_mask.hip",
       "interpolate_bicubic.hip", "hole_fill.hip"]
# the issue's sizes, then those of the stages' GPU tests and cases modules up to 257 x 131
SIZES = [(1, 1), (3, 2), (65, 5), (67, 9), (130, 3), (7, 5), (33, 17), (64, 64), (257, 131)]
FACTORS = cases.DYADIC_FACTORS + cases.INEXACT_FACTORS + cases.LIMIT_FACTORS
MATCH = [0, 48, 1020]


def fields(w, h, seed):
    """(name, prev, curr, mv): the GPU test's random field and the end fields on the same frames."""
    prev, curr, mv = cases.field("random", w, h, seed)
    yield "random", prev, curr, mv
    for name, f in end_fields(w, h, seed):
        yield name, prev, curr, f
    p2, c2, m2 = cases.field("piecewise", w, h, seed)
    yield "piecewise", p2, c2, m2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return kit.build(tmp_path_factory, request.param, "compensated_on_host", HIP)


@pytest.fixture(scope="module")
def thread_program(tmp_path_factory):
    return kit.build(tmp_path_factory, "thread", "compensated_on_host", HIP)


def check(cs, program, wants):
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert len(got) == 1
        assert (got[0] == want).all(), f"{label}: {kit.first_bad(got[0], want)}"


def test_compensated_and_masked_equal_their_models(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep(SIZES):
        rng = np.random.default_rng(k)
        for name, prev, curr, mv in fields(w, h, 13 * k + 5):
            for j in range(2 if w * h < 5000 else 1):
                t, ms = FACTORS[n % len(FACTORS)], MATCH[(n // 2) % 3]
                n += 1
                B = lambda a, unit: cs.buffer(a, lay, unit)
                out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
                cs.add(["mc", w, h, f32(t), ms, 0, B(prev, 4), B(curr, 4), B(mv, 2), out], [meta], f"mc {w}x{h} {lay} {name} t={t} ms={ms}")
                wants.append(mc_model.interpolate_compensated(prev, curr, mv, t, ms))
                # the masked pair: a random mask, all static, all clear
                mask = [np.where(rng.random((h, w)) < 0.3, rng.integers(1, 256, (h, w)), 0).astype(np.uint8), np.full((h, w), 255, np.uint8),
                        np.zeros((h, w), np.uint8)][n % 3]
                out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
                cs.add(["masked", w, h, f32(t), ms, 0, B(prev, 4), B(curr, 4), B(mv, 2), cs.buffer(mask, lay, 1), out], [meta],
                       f"masked {w}x{h} {lay} {name} mask {n % 3} t={t} ms={ms}")
                wants.append(overlay_model.interpolate_masked(prev, curr, mv, mask, t, ms))
    check(cs, program, wants)


def test_hand_made_cases_equal_their_models(program, tmp_path):
    """The cases modules' own inputs: the walk's reach, collisions, projections outside, the overlay rules."""
    cs, wants = kit.Cases(str(tmp_path)), []
    hand = [(*cases.mc_collision(textured_frames=True)[:3], 1020), (*cases.mc_unmatched_source(), 199), (*cases.mc_projection_outside(textured_frames=True), 1020),
            (*cases.mc_revealed_and_covered()[:3], 0), (*cases.mc_row_projected_to_the_top(), 1020), (*cases.mc_walk_reach()[:3], cases.WALK_REACH_MATCH_SAD)]
    for k, (prev, curr, mv, ms) in enumerate(hand):
        h, w = prev.shape[:2]
        lay = kit.LAYOUTS[k % 3]
        for t in (0.5, 0.3):
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["mc", w, h, f32(t), ms, 0, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(mv, lay, 2), out], [meta], f"hand-made {k} t={t}")
            wants.append(mc_model.interpolate_compensated(prev, curr, mv, t, ms))
    for k, (name, (prev, curr, mv, mask, ms)) in enumerate(overlay_cases.hand_made().items()):
        h, w = prev.shape[:2]
        lay = kit.LAYOUTS[k % 3]
        out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
        cs.add(["masked", w, h, f32(0.5), ms, 0, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(mv, lay, 2), cs.buffer(mask, lay, 1), out],
               [meta], name)
        wants.append(overlay_model.interpolate_masked(prev, curr, mv, mask, 0.5, ms))
    check(cs, program, wants)


def test_extrapolation_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep(SIZES):
        for name, prev, curr, mv in fields(w, h, 7 * k + 3):
            a, ms = extrapolate_cases.FACTORS[n % len(extrapolate_cases.FACTORS)], extrapolate_cases.MATCH[(n // 2) % 3]
            n += 1
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["extrapolate", w, h, f32(a), ms, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(mv, lay, 2), out], [meta],
                   f"extrapolate {w}x{h} {lay} {name} ahead={a} ms={ms}")
            wants.append(extrapolate_model.extrapolate(prev, curr, mv, a, ms))
    check(cs, program, wants)


def test_bidirectional_and_consistency_equal_their_models(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep(SIZES):
        quads = [(kind, *bidir_cases.field(kind, w, h, 5 * k + 1)) for kind in ("random", "small", "piecewise")]
        prev, curr = quads[0][1:3]
        ends = list(end_fields(w, h, k))
        quads += [("ends", prev, curr, ends[0][1], ends[-1][1]), ("ends swapped", prev, curr, ends[-1][1], ends[0][1])]
        for name, prev, curr, fwd, bwd in quads:
            t, ms, tol = bidir_cases.FACTORS[n % len(bidir_cases.FACTORS)], bidir_cases.MATCH[(n // 2) % 3], bidir_cases.TOLERANCES[(n // 3) % 3]
            n += 1
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["bidir", w, h, f32(t), ms, tol, 0, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(fwd, lay, 2), cs.buffer(bwd, lay, 2), out],
                   [meta], f"bidir {w}x{h} {lay} {name} t={t} ms={ms} tol={tol}")
            wants.append(bidir_model.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol))
            out, meta = cs.output((h, w), np.uint8, lay, 1)
            cs.add(["consistency", w, h, tol, cs.buffer(fwd, lay, 2), cs.buffer(bwd, lay, 2), out], [meta], f"consistency {w}x{h} {lay} {name} tol={tol}")
            wants.append(bidir_model.consistency(fwd, bwd, tol))
    check(cs, program, wants)


def test_static_mask_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    for k, w, h, lay in sweep(SIZES):
        prev = cases.textured(w, h, k)
        curr = np.clip(prev.astype(np.int16) + np.random.default_rng(k).integers(-3, 4, prev.shape), 0, 255).astype(np.uint8)
        curr[::2, ::3] = prev[::2, ::3]
        for tol in (0, 6, 1020):
            out, meta = cs.output((h, w), np.uint8, lay, 1)
            cs.add(["static_mask", w, h, tol, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), out], [meta], f"static_mask {w}x{h} {lay} tol={tol}")
            wants.append(overlay_model.static_mask(prev, curr, tol))
    check(cs, program, wants)


def test_subpel_route_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep(SIZES + [(97, 61), (130, 9)]):
        prev, curr, mvq = subpel_cases.random_mvq(w, h, 3 * k + 2)
        for name, field in (("random", mvq), ("ends", end_fields_q(w, h, k))):
            t, ms = subpel_cases.FACTORS[n % len(subpel_cases.FACTORS)], MATCH[(n // 2) % 3]
            n += 1
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["subpel", w, h, f32(t), ms, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(field, lay, 4), out], [meta],
                   f"subpel {w}x{h} {lay} {name} t={t} ms={ms}")
            wants.append(subpel_model.interpolate(prev, curr, field, t, ms))
    check(cs, program, wants)


def test_the_other_stages_hand_made_cases_equal_their_models(program, tmp_path):
    """The hand-made inputs of bidir_cases, extrapolate_cases and subpel_cases -- built to point at and across the frame's edge --
    as their GPU tests run them, the three layouts in rotation."""
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0

    def add(op, params, frames, fields, unit, label, want):
        nonlocal n
        lay = kit.LAYOUTS[n % 3]
        n += 1
        h, w = frames[0].shape[:2]
        out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
        cs.add([op, w, h, *params, *[cs.buffer(f, lay, 4) for f in frames], *[cs.buffer(f, lay, unit) for f in fields], out], [meta], f"{label} {lay}")
        wants.append(want)

    for name, prev, curr, fwd, bwd, ms, tols in bidir_cases.shared_cases():
        for tol in tols:
            for t in (0.25, 0.5, 0.3):
                add("bidir", [f32(t), ms, tol, 0], [prev, curr], [fwd, bwd], 2, f"bidir {name} t={t} tol={tol}",
                    bidir_model.interpolate_bidirectional(prev, curr, fwd, bwd, t, ms, tol))
    prev, curr, fwd, bwd, blank = bidir_cases.walk_reach()
    for t in cases.WALK_REACH_FACTORS:
        for f, b in ((fwd, bwd), (blank, blank)):
            add("bidir", [f32(t), cases.WALK_REACH_MATCH_SAD, 0, 0], [prev, curr], [f, b], 2, f"bidir walk_reach t={t}",
                bidir_model.interpolate_bidirectional(prev, curr, f, b, t, cases.WALK_REACH_MATCH_SAD, 0))
    for name, prev, curr, mv, ms in extrapolate_cases.shared_cases():
        for a in extrapolate_cases.FACTORS:
            add("extrapolate", [f32(a), ms], [prev, curr], [mv], 2, f"extrapolate {name} ahead={a}", extrapolate_model.extrapolate(prev, curr, mv, a, ms))
    # the sub-pixel route: the collision on flat and on textured frames, revealed and covered, a refined pan, the known-answer
    # inputs' refined fields, and the anchor inputs, on which the route with 4 mv and the integer route give the same bytes
    z, zc, mvq, _, _ = subpel_cases.collision()
    textured = (cases.textured(8, 8, 61), cases.textured(8, 8, 62))
    for (prev, curr), ms in (((z, zc), 0), (textured, 1020)):
        add("subpel", [f32(subpel_cases.COLLISION_FACTOR), ms], [prev, curr], [mvq], 4, "subpel collision",
            subpel_model.interpolate(prev, curr, mvq, subpel_cases.COLLISION_FACTOR, ms))
    prev, curr, mvq, _ = subpel_cases.revealed_and_covered()
    add("subpel", [f32(0.5), 0], [prev, curr], [mvq], 4, "subpel revealed_and_covered", subpel_model.interpolate(prev, curr, mvq, 0.5, 0))
    for wq in subpel_cases.PANS[:2]:
        prev, curr, _ = subpel_cases.fractional_pan(97, 61, wq)
        mvq = subpel_model.refine(prev, curr, subpel_cases.pan_vectors(97, 61, wq), 1)
        for t in (0.25, 0.5, 0.7):
            add("subpel", [f32(t), 48], [prev, curr], [mvq], 4, f"subpel refined pan {wq} t={t}", subpel_model.interpolate(prev, curr, mvq, t, 48))
    for name in sorted(subpel_cases.KNOWN):
        prev, curr, mv, radius, _ = subpel_cases.KNOWN[name]()
        mvq = subpel_model.refine(prev, curr, mv, radius)
        add("subpel", [f32(0.5), 48], [prev, curr], [mvq], 4, f"subpel {name}", subpel_model.interpolate(prev, curr, mvq, 0.5, 48))
    k = 0
    for name, prev, curr, mv in subpel_cases.anchor_inputs():
        for t in subpel_cases.FACTORS:
            ms = subpel_cases.MATCH_SADS[k % 3]
            k += 1
            want = mc_model.interpolate_compensated(prev, curr, mv, t, ms)
            add("mc", [f32(t), ms, 0], [prev, curr], [mv], 2, f"anchor {name} t={t} ms={ms}, integer route", want)
            add("subpel", [f32(t), ms], [prev, curr], [4 * mv.astype(np.int16)], 4, f"anchor {name} t={t} ms={ms}, 4 mv", want)
            assert (subpel_model.interpolate(prev, curr, 4 * mv.astype(np.int16), t, ms) == want).all(), (name, t, ms)
    check(cs, program, wants)


# ---- the kernels with cross-lane operations: every lane a thread

FILL_SIZES = [(1, 1), (3, 2), (65, 5), (67, 9), (130, 3), (130, 70), (67, 131), (64, 64), (1, 200), (200, 1), (257, 131)]


def fill_plane_cases(cs, sizes, reaches):
    wants = []
    n = 0
    for k, w, h, lay in sweep(sizes):
        reach = reaches[k % len(reaches)]
        for name, K in fill_cases.patterns(w, h, reach):
            static = n % 2
            band = (0, 0, 5)[n % 3]                                  # the launcher's own band, and a small one: many band seams
            n += 1
            out, meta = cs.output((h, w), np.uint32, lay, 4)
            cs.add(["fill_plane", w, h, reach, static, band, cs.buffer(K, lay, 4), out], [meta], f"fill_plane {w}x{h} {lay} {name} reach={reach} static={static} band={band}")
            wants.append(fill_model.plane(K, reach, bool(static)))
    return wants


def test_fill_plane_equals_its_model(program, tmp_path):
    cs = kit.Cases(str(tmp_path))
    check(cs, program, fill_plane_cases(cs, FILL_SIZES, fill_cases.REACHES))


def test_fill_plane_under_the_thread_sanitizer(thread_program, tmp_path):
    """The row pass exchanges through the layer's mutex alone and the column pass shares nothing: clean by construction."""
    cs = kit.Cases(str(tmp_path))
    check(cs, thread_program, fill_plane_cases(cs, [(67, 9), (130, 3)], (16, 65)))


def test_routes_through_the_fill_plane_equal_their_models(program, tmp_path):
    """lfg_set_hole_reach's launchers: clear, project, both passes of the plane, the sampling kernel that reads it."""
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep([(1, 1), (3, 2), (65, 5), (67, 9), (130, 3), (33, 17), (97, 70)]):
        prev, curr, fwd, bwd = bidir_cases.field("random", w, h, 11 * k + 7)
        ends = list(end_fields(w, h, k))
        mask = np.where(np.random.default_rng(k).random((h, w)) < 0.3, 255, 0).astype(np.uint8)
        for name, f, b in (("random", fwd, bwd), ("ends", ends[0][1], ends[-1][1])):
            t, ms, reach = FACTORS[n % len(FACTORS)], MATCH[n % 3], (16, 32, 255, 1)[n % 4]
            n += 1
            B = lambda a, unit: cs.buffer(a, lay, unit)
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["mc", w, h, f32(t), ms, reach, B(prev, 4), B(curr, 4), B(f, 2), out], [meta], f"mc+plane {w}x{h} {lay} {name} t={t} ms={ms} reach={reach}")
            wants.append(fill_model.interpolate_compensated(prev, curr, f, t, reach, ms))
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["masked", w, h, f32(t), ms, reach, B(prev, 4), B(curr, 4), B(f, 2), B(mask, 1), out], [meta], f"masked+plane {w}x{h} {lay} {name} t={t} reach={reach}")
            wants.append(fill_model.interpolate_masked(prev, curr, f, mask, t, reach, ms))
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["bidir", w, h, f32(t), ms, 1, reach, B(prev, 4), B(curr, 4), B(f, 2), B(b, 2), out], [meta], f"bidir+plane {w}x{h} {lay} {name} t={t} reach={reach}")
            wants.append(fill_model.interpolate_bidirectional(prev, curr, f, b, t, reach, ms, 1))
    check(cs, program, wants)


def test_bicubic_routes_equal_their_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    factors = bicubic_cases.FACTORS + [bicubic_cases.PHASE_FACTOR]
    for k, w, h, lay in sweep(bicubic_cases.SIZES + [(67, 9), (130, 3)]):
        for name in bicubic_cases.SCENES:
            prev, curr, mvq, mv = bicubic_cases.scene(name, w, h, 31 * k + len(name))
            if name == "full_range":
                mvq, mv = (end_fields_q(w, h, k), list(end_fields(w, h, k))[0][1]) if k % 2 else (mvq, mv)
            t, ms = factors[n % len(factors)], bicubic_cases.MATCH_SADS[(n // 2) % 3]
            n += 1
            for op, field, unit in (("bicubic", mv, 2), ("subpel_bicubic", mvq, 4)):
                out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
                cs.add([op, w, h, f32(t), ms, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(field, lay, unit), out], [meta],
                       f"{op} {w}x{h} {lay} {name} t={t} ms={ms}")
                wants.append(bicubic_model.interpolate(prev, curr, field, t, ms))
    for name, field in bicubic_cases.shortcut_fields().items():           # the ballot's shortcut both ways
        h, w = field.shape[:2]
        prev, curr = bicubic_cases.soft_noise(w, h, 1), bicubic_cases.soft_noise(w, h, 2)
        out, meta = cs.output((h, w, 4), np.uint8, "poisoned", 4)
        cs.add(["subpel_bicubic", w, h, f32(0.5), 1020, cs.buffer(prev, "poisoned", 4), cs.buffer(curr, "poisoned", 4), cs.buffer(field, "poisoned", 4), out],
               [meta], f"shortcut {name}")
        wants.append(bicubic_model.interpolate(prev, curr, field, 0.5, 1020))
    check(cs, program, wants)
