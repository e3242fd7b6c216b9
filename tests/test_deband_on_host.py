"""deband.hip run on the CPU (tests/cpp/deband_on_host.cpp over tests/cpp/hip_on_host): the file compiled by g++ as it is, its
own launch_deband on frames that are each their own allocation ending where the last row ends -- tight, with ASan-poisoned row
padding at 8- and at 16-byte pitches (the latter is the 16-byte route with its remainder launch), and with a pitch that is
only 4-byte aligned -- and every output byte held to tests/deband_model.py.  radius * iterations goes up to 128, so on the small
sizes every tap clamps.  Built plainly and with -fsanitize=address,undefined; the sanitized code is always the stand-alone
program.  CPU only."""
import numpy as np
import pytest

from tests import deband_model as dm, on_host_kit as kit

SIZES = [(1, 1), (3, 2), (65, 5), (67, 9), (130, 3), (257, 33)]
THRESHOLDS, RADII, GRAINS, SEEDS = (0, 4, 64), (1, 16, 32), (0, 3, 16), (0, 1, 0xFFFFFFFF, 20240229)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    return kit.build(tmp_path_factory, request.param, "deband_on_host", ["deband.hip"])


def run(program, tmp_path, cases):
    """cases: (frame, layout, iterations, threshold, radius, grain, seed).  Every output against the model."""
    cs, wants = kit.Cases(str(tmp_path)), []
    for frame, lay, I, T, R, G, seed in cases:
        h, w = frame.shape[:2]
        out, meta = cs.output((h, w, 4), np.uint8, lay, 4)
        cs.add(["deband", w, h, I, T, R, G, seed, cs.buffer(frame, lay, 4), out], [meta], f"{w}x{h} {lay} I={I} T={T} R={R} G={G} seed={seed}")
        wants.append(dm.deband(frame, I, T, R, G, seed))
    for (label, _), got, want in zip(cs.outputs, cs.run(program), wants):
        assert (got[0] == want).all(), (label, kit.first_bad(got[0], want))


def test_every_size_and_layout_equals_the_model(program, tmp_path):
    """Every size under every layout and every I, the other parameters rotating through their lists."""
    cases, k = [], 0
    for w, h in SIZES:
        frame = dm.scene(w, h, 31 * w + h)
        for lay in kit.RECORD_LAYOUTS:
            for I in range(1, dm.MAX_ITERATIONS + 1):
                cases.append((frame, lay, I, THRESHOLDS[k % 3], RADII[(k // 3) % 3], GRAINS[(k // 2) % 3], SEEDS[k % 4]))
                k += 1
    run(program, tmp_path, cases)


def test_every_tap_clamps_at_the_largest_reach(program, tmp_path):
    """R = 32 at I = 4 reaches 128 pixels: further than every size here but the widest is wide, and further than all are high."""
    cases = []
    for k, (w, h) in enumerate(SIZES):
        for lay in ("poisoned16", "sentinel"):
            for T, G in ((64, 0), (4, 16), (64, 16)):
                cases.append((dm.scene(w, h, 7 + k), lay, 4, T, 32, G, SEEDS[(k + T) % 4]))
    run(program, tmp_path, cases)


def test_the_ends_of_every_range_on_noise(program, tmp_path):
    """Random bytes, 0 and 255 among them: sums at both ends, the clamp of v + n at 0 and at 255 under the largest grain."""
    rng = np.random.default_rng(11)
    frame = rng.choice(np.array([0, 1, 2, 3, 127, 128, 252, 253, 254, 255], np.uint8), (9, 67, 4))
    cases = [(frame, lay, I, T, R, G, 5) for lay in ("poisoned16", "sentinel") for I in (1, 4) for T in (0, 64) for R in (1, 32) for G in (0, 16)]
    run(program, tmp_path, cases)
