"""csrc/lfg_resample.hpp without a GPU: tests/cpp/resample_on_host.cpp compiles the tile plan and the two phase bodies of the
resample kernel for the CPU with g++ alone and runs a launch as loops over tiles and threads, phase 1 for all threads and then
phase 2; what comes out is held, byte for byte, to the CPU model (tests/resample_model.py) on the shapes and layouts of
tests/test_gpu_resample.py, with a sentinel around every row.  The tables are the model's own.  CPU only."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import resample_model as rm
from tests import sharpen_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = rm.SENTINEL


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("resample_on_host") / "resample_on_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "resample_on_host.cpp"), "-o", str(out)])
    return out


@functools.lru_cache(maxsize=None)
def table(filt, n_in, n_out):
    return rm.table(filt, n_in, n_out)


def laid_out(rows, pitch):
    n_rows, n = rows.shape
    flat = np.full((n_rows - 1) * pitch + n, SENTINEL, np.uint8)
    np.lib.stride_tricks.as_strided(flat, (n_rows, n), (pitch, 1))[...] = rows
    return flat


def run(program, frame, ow, oh, filt, in_layout, out_layout):
    """(the program's output rows, its plan (T, span))."""
    (in_pitch, in_lead), (out_pitch, out_lead) = in_layout, out_layout
    h, w = frame.shape[:2]
    d = program.parent
    laid_out(frame.reshape(h, w * 4), in_pitch).tofile(d / "in.bin")
    for name, t in (("tx.bin", table(filt, w, ow)), ("ty.bin", table(filt, h, oh))):
        with open(d / name, "wb") as f:
            f.write(t[0].astype(np.int32).tobytes() + t[1].astype(np.uint32).tobytes() + t[2].astype(np.int16).tobytes())
    p = subprocess.run([str(a) for a in (program, w, h, ow, oh, in_pitch, out_pitch, in_lead, out_lead, d / "in.bin", d / "out.bin",
                                         d / "tx.bin", d / "ty.bin")], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    flat = np.fromfile(d / "out.bin", np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[out_lead:], (oh, ow * 4), (out_pitch, 1))
    rows = view.copy()
    view[...] = SENTINEL
    assert (flat == SENTINEL).all(), "bytes outside the rows were written"
    return rows.reshape(oh, ow, 4), tuple(int(v) for v in p.stdout.split())


def check(program, frame, ow, oh, filt, layout="dword"):
    h, w = frame.shape[:2]
    got, plan = run(program, frame, ow, oh, filt, rm.layouts(w)[layout], rm.layouts(ow)[layout])
    want = rm.resample_int(frame, table(filt, w, ow), table(filt, h, oh))
    assert (got == want).all(), (f"{w}x{h}->{ow}x{oh} {rm.NAMES[filt]} layout {layout}: {int((got != want).sum())} bytes differ, "
                                 f"first at {np.argwhere(got != want)[:3].tolist()}")
    assert plan == rm.plan_rows(*table(filt, h, oh)[:2]), "the header's plan is not the model's"
    return plan


@pytest.mark.parametrize("shape", rm.SHAPES, ids=["{}x{}-{}x{}".format(*s) for s in rm.SHAPES])
def test_phases_on_the_host_equal_the_model(program, shape):
    w, h, ow, oh = shape
    for filt in rm.FILTERS:
        for k, layout in enumerate(rm.layouts(w)):
            check(program, sm.smooth_scene(w, h, 100 * w + h), ow, oh, filt, layout)
            if k != 1:
                check(program, sm.noise(w, h, 200 * w + h + filt), ow, oh, filt, layout)


def test_every_output_height_around_the_tile(program):
    """13 x 40 -> 17 x h for h = 1 .. 2 T + 1: a tile one row short, full, one row into the next, two tiles and a row.  (The
    lowest heights are refused under the wider filters -- 40 : 1 is more than 64 taps -- and nearest takes them all.)"""
    frame = sm.noise(13, 40, 7)
    for filt in (rm.NEAREST, rm.BILINEAR, rm.LANCZOS3):
        heights = [oh for oh in range(1, 2 * 16 + 2) if table(filt, 40, oh) is not None]
        assert heights == list(range({rm.NEAREST: 1, rm.BILINEAR: 2, rm.LANCZOS3: 4}[filt], 34))
        for oh in heights:
            T, _ = check(program, frame, 17, oh, filt)
            assert T == 16


@pytest.mark.parametrize("rows", [4, 2, 1])
def test_downscales_that_force_few_rows_per_tile(program, rows):
    w, h, ow, oh = rm.SMALL_T[rows]
    frame = sm.noise(w, h, 30 + rows)
    assert check(program, frame, ow, oh, rm.LANCZOS3)[0] == rows
    for filt in rm.FILTERS:
        check(program, frame, ow, oh, filt)
        check(program, frame, ow, oh - 1, filt)                    # a last tile that is not full


def test_a_source_of_64_rows_fits_whole(program):
    """8 x 64 -> 8 x h: the whole source is one tile's worth of LDS rows, so T stays 16 at every ratio, 64 taps included."""
    frame = rm.binary_noise(8, 64, 11)
    for oh in (32, 13, 8, 7, 6):
        assert check(program, frame, 8, oh, rm.LANCZOS3)[0] == 16
