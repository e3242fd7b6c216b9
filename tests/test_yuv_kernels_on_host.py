"""csrc/yuv_convert.hip without a GPU: tests/cpp/yuv_kernels_on_host.cpp compiles both kernels for the CPU with g++ alone and runs
a launch as loops over blocks and threads; what comes out is held, byte for byte, to the CPU model (tests/yuv_model.py) on the
shapes of tests/test_gpu_yuv.py -- tight pitches, padded and misaligned ones (every item one quad), and bases and pitches that
allow the 8 x 2 items, at widths that leave 0 .. 3 quads behind them -- with a sentinel around every row.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import yuv_model as ym

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SHAPES = [(2, 2), (4, 2), (16, 2), (18, 6), (62, 34), (130, 4), (8, 2), (10, 2), (520, 6)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("yuv_on_host") / "yuv_kernels_on_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "yuv_kernels_on_host.cpp"), "-o", str(out)])
    return out


def laid_out(rows, pitch):
    n_rows, n = rows.shape
    flat = np.full((n_rows - 1) * pitch + n, SENTINEL, np.uint8)
    np.lib.stride_tricks.as_strided(flat, (n_rows, n), (pitch, 1))[...] = rows
    return flat


def rows_of(flat, lead, n_rows, n, pitch, what):
    view = np.lib.stride_tricks.as_strided(flat[lead:], (n_rows, n), (pitch, 1))
    rows = view.copy()
    view[...] = SENTINEL
    assert (flat == SENTINEL).all(), f"{what}: bytes outside the rows were written"
    return rows


def launch(program, direction, mode, w, h, pitches, leads, wide, data):
    matrix, rng, siting = mode
    to_rgb, to_yuv = ym.coefficients(matrix, rng)
    src, dst = program.parent / "in.bin", program.parent / "out.bin"
    src.write_bytes(data)
    args = [program, direction, siting, w, h, *pitches, *leads, wide, src, dst, *to_rgb, *to_yuv, ym.offset(rng)]
    p = subprocess.run([str(a) for a in args], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return np.fromfile(dst, np.uint8)


def check(program, w, h, mode, pitches, leads, wide):
    y_pitch, uv_pitch, rgba_pitch = pitches
    y, uv = ym.random_nv12(w, h, 7 * w + h)
    rgba = ym.random_rgba(w, h, w + h)
    what = f"{w}x{h} mode {mode} pitches {pitches} wide items {wide}"
    out = launch(program, 0, mode, w, h, pitches, leads, wide, laid_out(y, y_pitch).tobytes() + laid_out(uv.reshape(h // 2, w), uv_pitch).tobytes())
    got, want = rows_of(out, leads[2], h, w * 4, rgba_pitch, what).reshape(h, w, 4), ym.nv12_to_rgba(y, uv, *mode)
    assert (got == want).all(), f"NV12 -> RGBA {what}: first at {np.argwhere(got != want)[:3].tolist()}"
    check_to_nv12(program, rgba, mode, pitches, leads, wide)


def check_to_nv12(program, rgba, mode, pitches, leads, wide):
    (h, w), (y_pitch, uv_pitch, rgba_pitch) = rgba.shape[:2], pitches
    what = f"{w}x{h} mode {mode} pitches {pitches} wide items {wide}"
    out = launch(program, 1, mode, w, h, pitches, leads, wide, laid_out(rgba.reshape(h, w * 4), rgba_pitch).tobytes())
    y_bytes = leads[0] + (h - 1) * y_pitch + w
    got_y = rows_of(out[:y_bytes].copy(), leads[0], h, w, y_pitch, what)
    got_uv = rows_of(out[y_bytes:].copy(), leads[1], h // 2, w, uv_pitch, what).reshape(h // 2, w // 2, 2)
    want_y, want_uv = ym.rgba_to_nv12(rgba, *mode)
    assert (got_y == want_y).all(), f"RGBA -> NV12 luma {what}: first at {np.argwhere(got_y != want_y)[:3].tolist()}"
    assert (got_uv == want_uv).all(), f"RGBA -> NV12 chroma {what}: first at {np.argwhere(got_uv != want_uv)[:3].tolist()}"
    return got_uv


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_kernels_on_the_host_equal_the_model(program, w, h):
    for mode in ym.MODES:
        check(program, w, h, mode, (w, w, w * 4), (0, 0, 0), 0)                              # tight: every item one quad
        check(program, w, h, mode, (w + 2, w + 6, w * 4 + 4), (1, 2, 4), 0)                  # padded, nothing aligned
        check(program, w, h, mode, (w + 1, w + 6, w * 4 + 4), (0, 0, 0), 0)                  # an odd luma pitch: every second row pair odd
        if w >= 8:                                                                           # the 8 x 2 items and what is left of the row
            y_pitch, rgba_pitch = (w + 7) // 8 * 8 + 8, (w * 4 + 15) // 16 * 16 + 16
            check(program, w, h, mode, (y_pitch, y_pitch + 8, rgba_pitch), (8, 16, 32), w // 8)


@pytest.mark.parametrize("w,h", [(2, 2), (18, 6), (24, 4)], ids=["2x2", "18x6", "24x4"])
def test_saturated_blue_and_red_reach_the_upper_chroma_clamp(program, w, h):
    """The one clamp of RGBA -> NV12 that can fire: uniform quads of pure blue and pure red under the full range (128 + 128)."""
    layouts = [((w, w, w * 4), (0, 0, 0), 0), ((w + 1, w + 6, w * 4 + 4), (0, 0, 0), 0)]
    if w >= 8:
        layouts.append((((w + 7) // 8 * 8 + 8, (w + 7) // 8 * 8 + 16, (w * 4 + 15) // 16 * 16 + 16), (8, 16, 32), w // 8))
    for matrix in ym.MATRICES:
        for siting in ym.SITINGS:
            for layout in layouts:
                blue, red = ym.saturated_rgba(w, h, 900 + w)
                uv = check_to_nv12(program, blue, (matrix, ym.FULL, siting), *layout)
                assert (uv[0, :, 0] == 255).all() and (uv[0, :, 1] < 128).all()
                uv = check_to_nv12(program, red, (matrix, ym.FULL, siting), *layout)
                assert (uv[0, :, 1] == 255).all() and (uv[0, :, 0] < 128).all()
