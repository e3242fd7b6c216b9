"""csrc/lfg_bicubic.hpp without a GPU: tests/cpp/bicubic_on_host.cpp compiles the table rule, the integer body and the conversion
of p for the CPU with g++ alone and runs them on the shared cases' frames; what comes out is held, bit for bit, to the CPU model
(tests/bicubic_model.py).  The program is built twice, plainly and with -fsanitize=address,undefined (it has its own main): a
footprint that left its clamp would be a read out of an allocation of exactly the frame's size, and a shift or a product that
left 32 bits would be reported.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import bicubic_cases as bc
from tests import bicubic_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
SIZES = [(1, 1), (2, 2), (3, 5), (65, 5)]          # 1 x 1 and 2 x 2: every footprint clamps on all sides


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("bicubic_on_host_" + request.param) / "bicubic_on_host"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "bicubic_on_host.cpp"), "-o", str(out)]
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
    return p.stdout


def positions(w, h, seed):
    """Every phase on both axes around every texel of a small frame's corners, positions outside the image on every side (the
    clamp), the fraction that rounds to 1.0f, and random ones."""
    rng = np.random.default_rng(seed)
    grid = [(x + 0.5 + px / 64.0, y + 0.5 + py / 64.0) for x in (-2, 0, w - 1) for y in (-2, 0, h - 1)
            for px in range(0, 64, 3) for py in range(0, 64, 5)]
    sweep = [(0.5 + k / 64.0, h - 0.5 - k / 64.0) for k in range(-64, 129)]
    tiny = float(np.float32(0.5) - np.float32(2.0 ** -25))
    far = [(-300.25, 0.5), (w + 300.75, h + 200.0), (0.0, 0.0), (float(w), float(h)), (tiny, tiny)]
    rand = rng.uniform(-4.0, max(w, h) + 4.0, (400, 2)).tolist()
    return np.array(grid + sweep + far + rand, np.float32)


@pytest.mark.parametrize("size", SIZES, ids=["{}x{}".format(*s) for s in SIZES])
def test_fetch_on_the_host_equals_the_model(program, size):
    w, h = size
    d = program.parent
    pos = positions(w, h, 7 * w + h)
    pos.tofile(d / "pos.bin")
    for name in bc.SCENES:
        prev, curr, _, _ = bc.scene(name, w, h, 5)
        for img in (prev, curr):
            np.ascontiguousarray(img).tofile(d / "img.bin")
            run(program, "fetch", w, h, d / "img.bin", d / "pos.bin", d / "out.bin")
            got = np.fromfile(d / "out.bin", np.float32).reshape(-1, 4)
            want = np.stack([bm.fetch(img, float(px), float(py)) for px, py in pos])
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (name, np.argwhere(got != want)[:3].tolist())


def test_conversion_of_p_is_the_rounded_quotient_for_every_p(program):
    """Exhaustive, as the byte conversion is held for its 256 values: all 65,281 values of p."""
    assert int(run(program, "convert")) == 0


def test_rows_on_the_host_are_the_rule(program):
    out = program.parent / "table.bin"
    run(program, "table", out)
    rows = np.fromfile(out, np.int32).reshape(65, 4)
    assert (rows[:64] == bm.weights()).all()
    assert tuple(rows[64]) == (0, 0, 16384, 0)
