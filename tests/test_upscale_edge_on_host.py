"""The phase bodies of csrc/lfg_upscale_edge.hpp without a GPU: tests/cpp/upscale_edge_on_host.cpp compiles them for the CPU with
g++ alone and runs a launch as loops over tiles and threads, phase 1 for all threads and then phase 2; what comes out is held,
byte for byte, to the CPU model (tests/edge_model.py), with a sentinel around every row.  The program is built twice, plainly and
with -fsanitize=address,undefined (it has its own main): a coordinate that escaped its clamp, or a bracket outside its tile's
LDS words, would be a read out of an allocation of exactly the right size.  Positions and shapes are the model's own.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import edge_model as em
from tests import resample_model as rm
from tests.test_resample_on_host import SENTINEL, laid_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every read clamped; a small ragged ratio; exact 2x; near 1 : 1, the widest source span; across the 64-column tile, ragged, twice;
# every pixel in one bracket; an odd output width; one axis equal, the other, both; more than one tile of rows
SHAPES = [(1, 1, 4, 3), (5, 3, 11, 8), (13, 7, 26, 14), (13, 7, 17, 10), (40, 9, 130, 20), (67, 9, 130, 20), (2, 2, 131, 67), (33, 5, 65, 9),
          (24, 16, 48, 16), (24, 16, 24, 32), (24, 16, 24, 16), (130, 37, 131, 38)]
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("upscale_edge_on_host_" + request.param) / "upscale_edge_on_host"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "upscale_edge_on_host.cpp"), "-o", str(out)]
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(command)
    em.shapes().astype(np.int16).tofile(out.parent / "shapes.bin")
    return out


def run(program, frame, ow, oh, layout):
    h, w = frame.shape[:2]
    (in_pitch, in_lead), (out_pitch, out_lead) = rm.layouts(w)[layout], rm.layouts(ow)[layout]
    d = program.parent
    laid_out(frame.reshape(h, w * 4), in_pitch).tofile(d / "in.bin")
    for name, (base, frac) in (("px.bin", em.positions(w, ow)), ("py.bin", em.positions(h, oh))):
        with open(d / name, "wb") as f:
            f.write(base.astype(np.int32).tobytes() + frac.astype(np.uint8).tobytes())
    p = subprocess.run([str(a) for a in (program, w, h, ow, oh, in_pitch, out_pitch, in_lead, out_lead, d / "in.bin", d / "out.bin",
                                         d / "px.bin", d / "py.bin", d / "shapes.bin")], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    flat = np.fromfile(d / "out.bin", np.uint8)
    view = np.lib.stride_tricks.as_strided(flat[out_lead:], (oh, ow * 4), (out_pitch, 1))
    rows = view.copy()
    view[...] = SENTINEL
    assert (flat == SENTINEL).all(), "bytes outside the rows were written"
    return rows.reshape(oh, ow, 4)


def check(program, frame, ow, oh, layout="dword"):
    h, w = frame.shape[:2]
    got, want = run(program, frame, ow, oh, layout), em.upscale(frame, ow, oh)
    assert (got == want).all(), (f"{w}x{h}->{ow}x{oh} layout {layout}: {int((got != want).sum())} bytes differ, "
                                 f"first at {np.argwhere(got != want)[:3].tolist()}")


@pytest.mark.parametrize("shape", SHAPES, ids=["{}x{}-{}x{}".format(*s) for s in SHAPES])
def test_phases_on_the_host_equal_the_model(program, shape):
    w, h, ow, oh = shape
    for frame, layout in zip((em.binary_noise(w, h, 100 * w + h), em.random_bytes(w, h, 200 * w + h), em.diagonal_edge(w, h)), rm.layouts(w)):
        check(program, frame, ow, oh, layout)
