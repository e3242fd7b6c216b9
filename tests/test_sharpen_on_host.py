"""csrc/sharpen.hip without a GPU: tests/cpp/sharpen_on_host.cpp compiles both kernels for the CPU with g++ alone and runs the
launches of lfg_sharpen as loops over blocks and threads; what comes out is held, byte for byte, to the CPU model
(tests/sharpen_model.py) on the shapes and layouts of tests/test_gpu_sharpen.py, with a sentinel around every row.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import sharpen_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SHAPES = [(1, 1), (2, 1), (1, 3), (3, 2), (4, 1), (5, 3), (13, 7), (64, 4), (65, 4), (66, 4), (67, 9)]
STRENGTHS = (0, 1, 16, 37, 64)


def up16(n):
    return (n + 15) // 16 * 16


def layouts(w):
    """name -> ((in pitch, in lead), (out pitch, out lead), the kernels lfg_sharpen runs there)."""
    tight, odd, aligned = (w * 4, 0), (w * 4 + 4, 4), (up16(w * 4) + 16, 32)
    wide = ("wide" if w % 4 == 0 else "wide dword") if w >= 4 else "dword"
    return {"tight": (tight, tight, wide if w % 4 == 0 else "dword"),
            "dword": (odd, odd, "dword"),
            "aligned": (aligned, (up16(w * 4) + 32, 16), wide),
            "in-aligned": (aligned, odd, "dword"),
            "out-aligned": (odd, aligned, "dword")}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("sharpen_on_host") / "sharpen_on_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sharpen_on_host.cpp"), "-o", str(out)])
    return out


@pytest.fixture(scope="module")
def strip_rows(program):
    return int(subprocess.check_output([str(program), "--rows"], text=True))


def laid_out(rows, pitch):
    n_rows, n = rows.shape
    flat = np.full((n_rows - 1) * pitch + n, SENTINEL, np.uint8)
    np.lib.stride_tricks.as_strided(flat, (n_rows, n), (pitch, 1))[...] = rows
    return flat


def run(program, frame, strength, layout):
    (in_pitch, in_lead), (out_pitch, out_lead), kernels = layout
    h, w = frame.shape[:2]
    src, dst = program.parent / "in.bin", program.parent / "out.bin"
    laid_out(frame.reshape(h, w * 4), in_pitch).tofile(src)
    p = subprocess.run([str(a) for a in (program, w, h, in_pitch, out_pitch, in_lead, out_lead, strength, src, dst)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    assert p.stdout.strip() == kernels, (p.stdout, kernels)
    flat = np.fromfile(dst, np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[out_lead:], (h, w * 4), (out_pitch, 1))
    rows = view.copy()
    view[...] = SENTINEL
    assert (flat == SENTINEL).all(), "bytes outside the rows were written"
    return rows.reshape(h, w, 4)


def check(program, frame, strength, name, layout):
    got, want = run(program, frame, strength, layout), sm.sharpen(frame, strength)
    h, w = frame.shape[:2]
    assert (got == want).all(), f"{w}x{h} strength {strength} layout {name}: {int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[:3].tolist()}"


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_kernels_on_the_host_equal_the_model(program, w, h):
    for name, layout in layouts(w).items():
        for k, strength in enumerate(STRENGTHS):
            check(program, sm.smooth_scene(w, h, 100 * w + h), strength, name, layout)
            if k % 2 == 0:
                check(program, sm.noise(w, h, 200 * w + h + k), strength, name, layout)


@pytest.mark.parametrize("w", [5, 67])
def test_every_height_around_the_strip_length(program, strip_rows, w):
    """1 .. 2 R + 1 rows: a strip that is all halo, one short of full, full, one row into the next, two strips and a row."""
    for h in range(1, 2 * strip_rows + 2):
        for name in ("dword", "aligned"):
            check(program, sm.smooth_scene(w, h, 300 * w + h), 37, name, layouts(w)[name])
            check(program, sm.noise(w, h, 400 * w + h), 64, name, layouts(w)[name])


def test_impulses(program):
    for frame in sm.impulses():
        for name, layout in layouts(3).items():
            check(program, frame, 64, name, layout)
