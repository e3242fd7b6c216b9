"""The window-cost kernels and the denoiser run on the CPU (tests/cpp/window_cost_on_host.cpp over tests/cpp/hip_on_host):
motion_refine.hip, motion_expand.hip (with frame_halve), motion_subpel.hip and denoise.hip compiled by g++ as they are, their own
launch_* functions, every frame and vector field its own allocation that ends where its last row ends -- tight, with
ASan-poisoned row padding, and with a pitch that is only as aligned as the call asks for -- and every output byte held to the
model its GPU test holds it to.  Built plainly, with -fsanitize=address,undefined, and, for the two kernels that stage a tile in
LDS behind a barrier, with -fsanitize=thread on two sizes.  The sanitized code is always the stand-alone program.  CPU only."""
import numpy as np
import pytest

from tests import cases, denoise_cases as dc, denoise_model, expand_cases, expand_model, on_host_kit as kit, refine_model, subpel_cases, subpel_model
from tests.on_host_kit import end_fields, sweep

HIP = ["motion_refine.hip", "motion_expand.hip", "motion_subpel.hip", "denoise.hip"]
# the issue's sizes, then those of the stages' GPU tests and cases modules up to 257 x 131
SIZES = [(1, 1), (3, 2), (65, 5), (67, 9), (130, 3), (2, 2), (7, 5), (33, 17), (64, 64), (97, 61), (257, 131)]
RADII = (0, 1, 2)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return kit.build(tmp_path_factory, request.param, "window_cost_on_host", HIP)


@pytest.fixture(scope="module")
def thread_program(tmp_path_factory):
    return kit.build(tmp_path_factory, "thread", "window_cost_on_host", HIP)


def check(cs, program, wants):
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert (got[0] == want).all(), f"{label}: {kit.first_bad(got[0], want)}"


def refine_fields(w, h, seed):
    """(name, prev, curr, mv): test_gpu_refine's fields that need no estimator, and the end fields on noisy frames."""
    for kind in ("random", "piecewise", "uniform"):
        yield (kind, *cases.field(kind, w, h, seed))
    prev, curr, _ = subpel_cases.random_vectors(w, h, seed)
    for name, f in end_fields(w, h, seed):
        yield name, prev, curr, f


def refine_and_expand_cases(cs, sizes):
    wants = []
    n = 0
    for k, w, h, lay in sweep(sizes):
        wl, hl = expand_model.low_size(w, h)
        for name, prev, curr, mv in refine_fields(w, h, 13 * k + 5):
            radius = RADII[n % 3]
            n += 1
            out, meta = cs.output((h, w, 2), np.int8, lay, 2)
            cs.add(["refine", w, h, radius, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(mv, lay, 2), out], [meta],
                   f"refine {w}x{h} {lay} {name} radius={radius}")
            wants.append(refine_model.refine(prev, curr, mv, radius))
            low = np.ascontiguousarray(mv[:hl, :wl])
            out, meta = cs.output((h, w, 2), np.int8, lay, 2)
            cs.add(["expand", w, h, radius, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(low, lay, 2), out], [meta],
                   f"expand {w}x{h} {lay} {name} radius={radius}")
            wants.append(expand_model.expand(prev, curr, low, radius))
    return wants


def test_refine_and_expand_equal_their_models(program, tmp_path):
    cs = kit.Cases(str(tmp_path))
    wants = refine_and_expand_cases(cs, SIZES)
    for radius in RADII:                                              # the hand-made cases of tests/cases.py
        hand = [cases.refine_straight_edge(radius, False)[:3], cases.refine_straight_edge(radius, True)[:3], cases.refine_cost_before_length()[:3],
                cases.refine_candidates_outside()[:3], cases.refine_prev_outside_zero()[:3]]
        for k, (prev, curr, mv) in enumerate(hand):
            h, w = prev.shape[:2]
            lay = kit.LAYOUTS[(k + radius) % 3]
            out, meta = cs.output((h, w, 2), np.int8, lay, 2)
            cs.add(["refine", w, h, radius, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(mv, lay, 2), out], [meta], f"hand-made {k} radius={radius}")
            wants.append(refine_model.refine(prev, curr, mv, radius))
    check(cs, program, wants)


def test_named_cases_of_expand_and_subpel_equal_their_models(program, tmp_path):
    """expand_cases.CASES (saturation: every candidate outside the image; parity; the neighbours; the tie order) and
    subpel_cases.KNOWN (off_image and flat among them) at every radius, as their GPU tests run them, with the literal answers."""
    cs, wants, literal = kit.Cases(str(tmp_path)), [], []
    n = 0
    for name in sorted(expand_cases.CASES):
        prev, curr, low, at, want, _ = expand_cases.CASES[name]()
        h, w = prev.shape[:2]
        for radius in RADII:
            lay = kit.LAYOUTS[n % 3]
            n += 1
            out, meta = cs.output((h, w, 2), np.int8, lay, 2)
            cs.add(["expand", w, h, radius, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(low, lay, 2), out], [meta], f"expand {name} radius={radius} {lay}")
            wants.append(expand_model.expand(prev, curr, low, radius))
            literal.append({at: want})
    for name in sorted(subpel_cases.KNOWN):
        prev, curr, mv, own_radius, known = subpel_cases.KNOWN[name]()
        h, w = prev.shape[:2]
        for radius in RADII:
            lay = kit.LAYOUTS[n % 3]
            n += 1
            out, meta = cs.output((h, w, 2), np.int16, lay, 4)
            cs.add(["subpel", w, h, radius, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(mv, lay, 2), out], [meta], f"subpel {name} radius={radius} {lay}")
            wants.append(subpel_model.refine(prev, curr, mv, radius))
            literal.append(known if radius == own_radius else {})
    for (label, _), got, want, known in zip(cs.outputs, cs.run(program), wants, literal):
        assert (got[0] == want).all(), f"{label}: {kit.first_bad(got[0], want)}"
        for (x, y), v in known.items():
            assert tuple(int(c) for c in got[0][y, x]) == tuple(v), (label, x, y)


def test_refine_and_expand_under_the_thread_sanitizer(thread_program, tmp_path):
    """A tile cell read before the barrier that orders it is a report here; with the barrier in place there is none."""
    cs = kit.Cases(str(tmp_path))
    check(cs, thread_program, refine_and_expand_cases(cs, [(67, 9), (130, 3)]))


def test_halve_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    for k, w, h, lay in sweep(SIZES + [(3, 3), (17, 9), (96, 64)]):
        img = cases.textured(w, h, 7 * w + h)
        wl, hl = expand_model.low_size(w, h)
        out, meta = cs.output((hl, wl, 4), np.uint8, lay, 4)
        cs.add(["halve", w, h, cs.buffer(img, lay, 4), out], [meta], f"halve {w}x{h} {lay}")
        wants.append(expand_model.halve(img))
    check(cs, program, wants)


def test_subpel_refinement_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep(SIZES + [(130, 9)]):
        prev, curr, mv = subpel_cases.random_vectors(w, h, 3 * k + 1)
        ends = list(end_fields(w, h, k))
        for name, field in [("random", mv)] + (ends if w * h < 5000 else ends[:1]):      # the largest size: "ends" alone
            radius = RADII[n % 3]
            n += 1
            out, meta = cs.output((h, w, 2), np.int16, lay, 4)
            cs.add(["subpel", w, h, radius, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), cs.buffer(field, lay, 2), out], [meta],
                   f"subpel {w}x{h} {lay} {name} radius={radius}")
            wants.append(subpel_model.refine(prev, curr, field, radius))
    check(cs, program, wants)


def test_denoise_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep(dc.SHAPES + [(67, 9), (130, 3), (97, 61)]):
        curr = dc.noisy(dc.scene(w, h, k), 6, k + 1)
        mixed = dc.noisy(curr, 12, k + 3)
        mixed[:, : w // 2] = dc.random_frame(w, h, k + 4)[:, : w // 2]
        refs = [dc.noisy(dc.scene(w, h, k), 6, k + 2), mixed]
        fields = list(dc.fields(w, h, 20 * w + h).items()) + [("small", dc.small_field(w, h, k, 1))] + list(end_fields(w, h, k))
        for j, (name, field) in enumerate(fields):
            other = fields[(j + 1) % len(fields)][1]
            params = [(32, 192, 255)] + dc.EXTREMES
            tolerance, strength, limit = params[n % len(params)]
            count, radius = dc.COUNTS[n % 2], dc.RADII[(n // 2) % 3]
            n += 1
            words = ["denoise", w, h, count, radius, tolerance, strength, limit, cs.buffer(curr, lay, 4)]
            for r, m in list(zip(refs, (field, other)))[:count]:
                words += [cs.buffer(r, lay, 4), cs.buffer(m, lay, 2)]
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(words + [out], [meta], f"denoise {w}x{h} {lay} {name} count={count} radius={radius} ({tolerance}, {strength}, {limit})")
            wants.append(denoise_model.denoise(curr, refs[:count], [field, other][:count], radius, tolerance, strength, limit))
    check(cs, program, wants)
