"""The record kernels run on the CPU (tests/cpp/record_on_host.cpp over tests/cpp/hip_on_host): pair_stats.hip, frame_diff.hip,
frame_ssim.hip and levels.hip compiled by g++ as they are, their own launch_* functions at 1, 2 and 256 compute units, every
frame its own allocation that ends where its last row ends -- tight, with ASan-poisoned row padding (at 8- and at 16-byte
pitches: the 16-byte walks), and with a pitch that is only 4-byte aligned -- every record and map an allocation of exactly its
size, and every word held to the model its GPU test holds it to.  Built plainly and with -fsanitize=address,undefined; the
sanitized code is always the stand-alone program.  CPU only."""
import numpy as np
import pytest

from tests import cases, diff_model, levels_cases, levels_model, on_host_kit as kit, pair_model, ssim_model
from tests.on_host_kit import end_fields, f32, sweep

HIP = ["pair_stats.hip", "frame_diff.hip", "frame_ssim.hip", "levels.hip"]
SIZES = [(1, 1), (3, 2), (65, 5), (67, 9), (130, 3), (3, 5), (64, 48), (257, 33), (257, 131)]
SSIM_SIZES = [(8, 8), (11, 9), (67, 9), (130, 12), (64, 48), (257, 33)]          # the call takes frames of 8 x 8 and more
LAYOUTS = kit.RECORD_LAYOUTS
CUS = (1, 2, 256)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return kit.build(tmp_path_factory, request.param, "record_on_host", HIP)


def sweep4(sizes):
    k = 0
    for w, h in sizes:
        for lay in LAYOUTS:
            yield k, w, h, lay
            k += 1


def record_output(cs, words):
    return cs.output((1, words), np.uint64, "tight", 8)


def test_pair_match_and_cut_fallback_equal_their_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep4(SIZES):
        prev, curr, mv = cases.field("random", w, h, k)
        near = np.clip(prev.astype(np.int16) + np.random.default_rng(k).integers(-9, 10, prev.shape), 0, 255).astype(np.uint8)
        for name, c, field in [("random", curr, mv), ("near", near, np.zeros_like(mv))] + [(nm, near, f) for nm, f in end_fields(w, h, k)]:
            ms, cus = (0, 48, 1020)[n % 3], CUS[(n // 3) % 3]
            n += 1
            out, meta = record_output(cs, 3)
            cs.add(["pair", w, h, ms, cus, cs.buffer(prev, lay, 4), cs.buffer(c, lay, 4), cs.buffer(field, lay, 2), out], [meta],
                   f"pair {w}x{h} {lay} {name} ms={ms} cus={cus}")
            wants.append([np.array([pair_model.pair_stats(prev, c, field, ms)], np.uint64)])
        # the fallback on a record that cuts and on one that does not: a cut copies prev or curr, no cut leaves the outputs alone
        factors = [0.0, 0.3, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.5, 1.0][: 1 + k % 5]
        for stats, permille in (((w * h, 0, 0), 1000), ((w * h, w * h, 0), 1000), ((w * h, w * h // 2, 0), (0, 500, 501)[k % 3])):
            record = cs.buffer(np.array([stats], np.uint64), "tight", 8)
            outs = [cs.output((h, w, 4), np.uint8, lay, 4) for _ in factors]
            cs.add(["cut", w, h, permille, CUS[k % 3], len(factors), record, cs.buffer(prev, lay, 4), cs.buffer(curr, lay, 4), *[o[0] for o in outs],
                    *[f32(t) for t in factors]], [o[1] for o in outs], f"cut {w}x{h} {lay} {stats} permille={permille}")
            untouched = np.full((h, w, 4), kit.SENTINEL, np.uint8)
            wants.append(pair_model.fallback(prev, curr, factors) if pair_model.cut(stats, permille) else [untouched] * len(factors))
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert len(got) == len(want)
        for g, w_ in zip(got, want):
            assert (g == w_).all(), label


def words_of_diff(r):
    return np.array([[r[0], *r[1], *r[2]]], np.uint64)


def words_of_ssim(r):
    return np.array([[r[0], *[v & ((1 << 64) - 1) for v in r[1]], *r[2], r[3]]], np.uint64)


def test_frame_diff_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep4(SIZES):
        a, b = diff_model.graded(w, h, k)[:2] if k % 2 else (cases.textured(w, h, k), cases.textured(w, h, k + 1))
        for repeat in (1, 2):
            mask, cus = diff_model.MASKS[n % 4], CUS[(n // 2) % 3]
            n += 1
            out, meta = record_output(cs, 261)
            cs.add(["diff", w, h, mask, cus, repeat, cs.buffer(a, lay, 4), cs.buffer(b, lay, 4), out], [meta], f"diff {w}x{h} {lay} mask={mask} cus={cus} x{repeat}")
            r = diff_model.frame_diff(a, b, mask)
            wants.append(words_of_diff(r if repeat == 1 else diff_model.add(r, r)))
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert (got[0] == want).all(), (label, np.argwhere(got[0] != want)[:4].tolist())


def test_frame_ssim_equals_its_model(program, tmp_path):
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep4(SSIM_SIZES):
        pairs = list(ssim_model.scenes(w, h).items())
        name, (a, b) = pairs[k % len(pairs)]
        for repeat in (1, 2):
            mask, cus = ssim_model.MASKS[n % 4], CUS[(n // 2) % 3]
            n += 1
            out, meta = record_output(cs, 71)
            cs.add(["ssim", w, h, mask, cus, repeat, cs.buffer(a, lay, 4), cs.buffer(b, lay, 4), out], [meta], f"ssim {w}x{h} {lay} {name} mask={mask} cus={cus} x{repeat}")
            r = ssim_model.frame_ssim(a, b, mask)
            wants.append(words_of_ssim(r if repeat == 1 else ssim_model.add(r, r)))
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert (got[0] == want).all(), (label, np.argwhere(got[0] != want)[:4].tolist())


def flat(w, h):
    return np.full((h, w, 4), (17, 200, 3, 255), np.uint8)


def test_levels_equal_their_model(program, tmp_path):
    """Histogram, match and apply: random content, flat content (every lane of a wave on one bin) and a fade."""
    cs, wants = kit.Cases(str(tmp_path)), []
    n = 0
    for k, w, h, lay in sweep4(SIZES):
        frame = [cases.textured(w, h, k), flat(w, h), levels_cases.fade(cases.textured(w, h, k), 205, 0)][k % 3]
        for repeat in (1, 2):
            out, meta = record_output(cs, 1025)
            cs.add(["hist", w, h, CUS[n % 3], repeat, cs.buffer(frame, lay, 4), out], [meta], f"hist {w}x{h} {lay} content {k % 3} x{repeat}")
            n += 1
            rec = levels_model.histogram(frame)
            wants.append(levels_model.record_words(rec if repeat == 1 else levels_model.histogram(frame, rec))[None, :])
        base = cases.textured(w, h, k + 50)
        faded = levels_cases.fade(base, *levels_cases.FADES["gain230plus10"])
        rec_from, rec_to = levels_model.histogram(faded), levels_model.histogram(base if k % 4 else flat(w + 1, h))
        for min_shift in levels_cases.MIN_SHIFTS:
            m = levels_model.match(rec_from, rec_to, min_shift)
            out, meta = cs.output((1, 1560), np.uint8, "tight", 8)
            cs.add(["match", 1, 1, min_shift, cs.buffer(levels_model.record_words(rec_from)[None, :], "tight", 8),
                    cs.buffer(levels_model.record_words(rec_to)[None, :], "tight", 8), out], [meta], f"match {w}x{h} min_shift={min_shift}")
            wants.append(levels_model.map_bytes(m)[None, :])
        m = levels_model.match(rec_from, levels_model.histogram(base), 0)
        for mode, factor in [(levels_model.FORWARD, 0.0)] + [(levels_model.AT, t) for t in levels_cases.FACTORS[k % 2::2]]:
            out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
            cs.add(["apply", w, h, mode, levels_model.tq_of(factor), cs.buffer(faded, lay, 4), cs.buffer(levels_model.map_bytes(m)[None, :], "tight", 8), out],
                   [meta], f"apply {w}x{h} {lay} mode={mode} factor={factor}")
            wants.append(levels_model.apply(faded, m, mode, factor))
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert (got[0] == want).all(), (label, np.argwhere(got[0] != want)[:4].tolist())


def test_levels_match_on_hand_made_records(program, tmp_path):
    """levels_cases.record_pairs() -- single levels, disjoint ranges, unequal and zero pixel counts -- and the fades' records, as
    test_gpu_levels.py runs them: every byte of the map."""
    cs, wants = kit.Cases(str(tmp_path)), []
    pairs = dict(levels_cases.record_pairs())
    for name in levels_cases.FADES:
        prev, curr = levels_cases.faded_pan(64, 48, 5, name)
        pairs[name] = (levels_model.histogram(prev), levels_model.histogram(curr))
    for name, (a, b) in pairs.items():
        for min_shift in levels_cases.MIN_SHIFTS:
            out, meta = cs.output((1, 1560), np.uint8, "tight", 8)
            cs.add(["match", 1, 1, min_shift, cs.buffer(levels_model.record_words(a)[None, :], "tight", 8),
                    cs.buffer(levels_model.record_words(b)[None, :], "tight", 8), out], [meta], f"match {name} min_shift={min_shift}")
            wants.append(levels_model.map_bytes(levels_model.match(a, b, min_shift))[None, :])
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert (got[0] == want).all(), (label, np.argwhere(got[0] != want)[:4].tolist())
