"""The linear- and sigmoidal-light bodies of csrc/lfg_resample.hpp without a GPU: tests/cpp/light_on_host.cpp compiles them for the
CPU with g++ alone and runs a launch as loops over tiles and threads -- the staging of the tables for all threads, then phase 1,
then phase 2; what comes out is held, byte for byte, to the CPU model (tests/light_model.py), with a sentinel around every row.
The program is built twice, plainly and with -fsanitize=address,undefined (it has its own main): its LDS stand-in is exactly the
span * 512 + 1024 bytes the launch asks for, so a lookup past a table, or a row past the tile, would be an access outside an
allocation of exactly the right size.  Tables are the model's own.  CPU only."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import light_model as lm
from tests import resample_model as rm
from tests.test_resample_on_host import SENTINEL, laid_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = tuple(f for f in rm.FILTERS if f != rm.NEAREST)
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("light_on_host_" + request.param) / "light_on_host"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "light_on_host.cpp"), "-o", str(out)]
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


@functools.lru_cache(maxsize=None)
def light_tables(mode):
    return lm.tables(mode)


def modes(w, h, ow, oh):
    return lm.MODES if ow >= w and oh >= h else (lm.LINEAR,)


def run(program, frame, ow, oh, filt, mode, layout):
    """(the program's output rows, its plan (T, span))."""
    h, w = frame.shape[:2]
    (in_pitch, in_lead), (out_pitch, out_lead) = rm.layouts(w)[layout], rm.layouts(ow)[layout]
    d = program.parent
    laid_out(frame.reshape(h, w * 4), in_pitch).tofile(d / "in.bin")
    for name, t in (("tx.bin", table(filt, w, ow)), ("ty.bin", table(filt, h, oh))):
        with open(d / name, "wb") as f:
            f.write(t[0].astype(np.int32).tobytes() + t[1].astype(np.uint32).tobytes() + t[2].astype(np.int16).tobytes())
    forward, threshold = light_tables(mode)
    np.concatenate([forward, threshold, [0xFFFF]]).astype(np.uint16).tofile(d / "light.bin")
    p = subprocess.run([str(a) for a in (program, w, h, ow, oh, in_pitch, out_pitch, in_lead, out_lead, d / "in.bin", d / "out.bin",
                                         d / "tx.bin", d / "ty.bin", d / "light.bin")], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    flat = np.fromfile(d / "out.bin", np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[out_lead:], (oh, ow * 4), (out_pitch, 1))
    rows = view.copy()
    view[...] = SENTINEL
    assert (flat == SENTINEL).all(), "bytes outside the rows were written"
    return rows.reshape(oh, ow, 4), tuple(int(v) for v in p.stdout.split())


def check(program, frame, ow, oh, filt, mode, layout="dword"):
    h, w = frame.shape[:2]
    got, plan = run(program, frame, ow, oh, filt, mode, layout)
    want = lm.light(frame, ow, oh, filt, mode, table(filt, w, ow), table(filt, h, oh), light_tables(mode))
    assert (got == want).all(), (f"{w}x{h}->{ow}x{oh} {rm.NAMES[filt]} {lm.NAMES[mode]} layout {layout}: {int((got != want).sum())} bytes differ, "
                                 f"first at {np.argwhere(got != want)[:3].tolist()}")
    assert plan == rm.plan_rows(*table(filt, h, oh)[:2]), "the header's plan is not the model's"
    return plan


@pytest.mark.parametrize("shape", rm.SHAPES, ids=["{}x{}-{}x{}".format(*s) for s in rm.SHAPES])
def test_phases_on_the_host_equal_the_model(program, shape):
    w, h, ow, oh = shape
    noise, rand = rm.binary_noise(w, h, 100 * w + h), np.random.default_rng(200 * w + h).integers(0, 256, (h, w, 4)).astype(np.uint8)
    for mode in modes(*shape):
        for filt in FILTERS:
            for layout in rm.layouts(w):
                check(program, noise, ow, oh, filt, mode, layout)
            check(program, rand, ow, oh, filt, mode)
            check(program, rand, ow, oh, filt, mode, "tight")


@pytest.mark.parametrize("rows", [4, 2, 1])
def test_few_rows_per_tile(program, rows):
    """8 x 110 / 160 / 200 -> 8 x 20: the vertical table forces T = 4 / 2 / 1 under Lanczos-3.  The height shrinks: linear light
    only.  One row fewer leaves a last tile that is not full, and 200 -> 19 rows is 64 taps: a tile's rows are the whole 32 KiB,
    with the tables behind them."""
    w, h, ow, oh = rm.SMALL_T[rows]
    frame = np.random.default_rng(30 + rows).integers(0, 256, (h, w, 4)).astype(np.uint8)
    assert check(program, frame, ow, oh, rm.LANCZOS3, lm.LINEAR)[0] == rows
    for filt in FILTERS:
        check(program, frame, ow, oh, filt, lm.LINEAR)
        plan = check(program, frame, ow, oh - 1, filt, lm.LINEAR)
    assert rows != 1 or plan == (1, rm.LDS_ROWS), plan                # (Lanczos-3 is the last filter)
