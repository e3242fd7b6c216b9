"""csrc/lfg_levels.hpp without a GPU: tests/cpp/levels_on_host.cpp compiles the map rule and both apply bodies for the CPU with
g++ alone and runs them on the shared cases; what comes out is held, byte for byte, to the CPU model (tests/levels_model.py).  The
program is built twice, plainly and with -fsanitize=address,undefined (it has its own main): a table index or a record word out
of range would be a read out of an allocation of exactly the right size, and a product that left its type would be reported.
CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import levels_cases as lc
from tests import levels_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("levels_on_host_" + request.param) / "levels_on_host"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "levels_on_host.cpp"), "-o", str(out)]
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(command)
    return out


def run(program, *args):
    p = subprocess.run([str(program), *[str(a) for a in args]], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])


def record_pairs():
    pairs = dict(lc.record_pairs())
    for name in lc.FADES:
        prev, curr = lc.faded_pan(64, 48, 5, name)
        pairs[name] = (lm.histogram(prev), lm.histogram(curr))
    prev, curr = lc.pan(64, 48, 3)
    pairs["pan"] = (lm.histogram(prev), lm.histogram(curr))
    # counts that no frame a device holds reaches: the products of the gate and of shift_sum wrap as the header's 64 bits do
    huge = np.zeros((4, 256), np.uint64)
    huge[:, 3] = 1 << 61
    far = np.zeros((4, 256), np.uint64)
    far[:, 250] = 1 << 61
    pairs["huge"] = ((1 << 61, huge), (1 << 61, far))
    return pairs


@pytest.mark.parametrize("name", list(record_pairs()))
def test_match_on_the_host_equals_the_model(program, name):
    d = program.parent
    a, b = record_pairs()[name]
    lm.record_words(a).tofile(d / "from.bin")
    lm.record_words(b).tofile(d / "to.bin")
    for s in lc.MIN_SHIFTS:
        run(program, "match", d / "from.bin", d / "to.bin", s, d / "map.bin")
        got = np.fromfile(d / "map.bin", np.uint8)
        want = lm.map_bytes(lm.match(a, b, s))
        assert got.size == 1560 and (got == want).all(), (name, s, np.argwhere(got != want)[:4].ravel().tolist())


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (67, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_apply_on_the_host_equals_the_model(program, size):
    w, h = size
    d = program.parent
    prev, curr = lc.faded_pan(w, h, 5, "gain230plus10")
    active = lm.match(lm.histogram(lc.faded_pan(64, 48, 5)[0]), lm.histogram(lc.faded_pan(64, 48, 5)[1]), 0)
    inactive = lm.pair_map(*lc.pan(64, 48, 3), lc.THRESHOLD)
    assert active["active"] == 1 and inactive["active"] == 0
    for m in (active, inactive):
        lm.map_bytes(m).tofile(d / "map.bin")
        for frame in (prev, curr):
            np.ascontiguousarray(frame).tofile(d / "in.bin")
            for mode, factor in [(lm.FORWARD, 0.0)] + [(lm.AT, f) for f in lc.FACTORS]:
                run(program, "apply", w, h, d / "in.bin", d / "map.bin", mode, f"{np.float32(factor):.9g}", d / "out.bin")
                got = np.fromfile(d / "out.bin", np.uint8).reshape(h, w, 4)
                want = lm.apply(frame, m, mode, factor)
                assert (got == want).all(), (mode, factor, m["active"])
                if not m["active"]:
                    assert (got == frame).all()
