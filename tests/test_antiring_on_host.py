"""The anti-ringing phase bodies of csrc/lfg_resample.hpp without a GPU: tests/cpp/antiring_on_host.cpp compiles them for the CPU
with g++ alone and runs a launch as loops over tiles and threads, phase 1 for all threads and then phase 2; what comes out is
held, byte for byte, to the CPU model (tests/antiring_model.py), with a sentinel around every row.  The program is built twice,
plainly and with -fsanitize=address,undefined (it has its own main): a bracket that left its taps, or its tile's LDS rows, would
be a read out of an allocation of exactly the right size.  Tables and brackets are the model's own.  CPU only."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import antiring_model as am
from tests import resample_model as rm
from tests.test_resample_on_host import SENTINEL, laid_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# both axes grow; across the 64-column tile with a ragged last one; one axis grows; none does (both strengths 0: the plain bytes)
SHAPES = [(1, 1, 4, 3), (5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (40, 9, 130, 20), (2, 2, 131, 67), (33, 5, 65, 9), (67, 9, 130, 20),
          am.HORIZONTAL_ONLY, am.VERTICAL_ONLY, (24, 16, 24, 16), (37, 19, 12, 6)]
RINGING = tuple(f for f in rm.FILTERS if f != rm.NEAREST)
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("antiring_on_host_" + request.param) / "antiring_on_host"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "antiring_on_host.cpp"), "-o", str(out)]
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(command)
    return out


@functools.lru_cache(maxsize=None)
def table(filt, n_in, n_out):
    return rm.table(filt, n_in, n_out)


def run(program, frame, ow, oh, filt, strength, layout):
    """(the program's output rows, its plan (T, span))."""
    h, w = frame.shape[:2]
    (in_pitch, in_lead), (out_pitch, out_lead) = rm.layouts(w)[layout], rm.layouts(ow)[layout]
    sx, sy = am.strengths(filt, w, h, ow, oh, strength)
    d = program.parent
    laid_out(frame.reshape(h, w * 4), in_pitch).tofile(d / "in.bin")
    for name, t in (("tx.bin", table(filt, w, ow)), ("ty.bin", table(filt, h, oh))):
        with open(d / name, "wb") as f:
            f.write(t[0].astype(np.int32).tobytes() + t[1].astype(np.uint32).tobytes() + t[2].astype(np.int16).tobytes())
    paths = []
    for name, s, n_in, n_out in (("bx.bin", sx, w, ow), ("by.bin", sy, h, oh)):
        if s:
            np.concatenate(am.brackets(n_in, n_out)).astype(np.int32).tofile(d / name)
        paths.append(d / name if s else "-")
    p = subprocess.run([str(a) for a in (program, w, h, ow, oh, in_pitch, out_pitch, in_lead, out_lead, d / "in.bin", d / "out.bin",
                                         d / "tx.bin", d / "ty.bin", sx, sy, *paths)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    flat = np.fromfile(d / "out.bin", np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[out_lead:], (oh, ow * 4), (out_pitch, 1))
    rows = view.copy()
    view[...] = SENTINEL
    assert (flat == SENTINEL).all(), "bytes outside the rows were written"
    return rows.reshape(oh, ow, 4), tuple(int(v) for v in p.stdout.split())


def check(program, frame, ow, oh, filt, strength, layout="dword"):
    h, w = frame.shape[:2]
    got, plan = run(program, frame, ow, oh, filt, strength, layout)
    want = am.antiring(frame, ow, oh, filt, strength, table(filt, w, ow), table(filt, h, oh))
    assert (got == want).all(), (f"{w}x{h}->{ow}x{oh} {rm.NAMES[filt]} S {strength} layout {layout}: {int((got != want).sum())} bytes differ, "
                                 f"first at {np.argwhere(got != want)[:3].tolist()}")
    assert plan == rm.plan_rows(*table(filt, h, oh)[:2]), "the header's plan is not the model's"
    return plan


@pytest.mark.parametrize("shape", SHAPES, ids=["{}x{}-{}x{}".format(*s) for s in SHAPES])
def test_phases_on_the_host_equal_the_model(program, shape):
    w, h, ow, oh = shape
    noise, rand = rm.binary_noise(w, h, 100 * w + h), np.random.default_rng(200 * w + h).integers(0, 256, (h, w, 4)).astype(np.uint8)
    for filt in RINGING:
        for k, layout in enumerate(rm.layouts(w)):
            check(program, noise, ow, oh, filt, (64, 24, 1)[k], layout)
        check(program, rand, ow, oh, filt, 64)
        check(program, rand, ow, oh, filt, 33, "tight")
    check(program, noise, ow, oh, rm.NEAREST, 64)                         # both strengths 0


@pytest.mark.parametrize("rows", [4, 2, 1])
def test_few_rows_per_tile_while_the_width_grows(program, rows):
    """8 x 110 / 160 / 200 -> 16 x 20: the vertical table forces T = 4 / 2 / 1 under Lanczos-3 and the horizontal pass is
    anti-ringed.  One row fewer leaves a last tile that is not full."""
    w, h, ow, oh = am.SMALL_T_UP[rows]
    frame = rm.binary_noise(w, h, 30 + rows)
    assert check(program, frame, ow, oh, rm.LANCZOS3, 64)[0] == rows
    for filt in RINGING:
        check(program, frame, ow, oh, filt, 40)
        check(program, frame, ow, oh - 1, filt, 64)
