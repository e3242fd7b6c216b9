"""csrc/lfg_denoise.hpp without a GPU: tests/cpp/denoise_on_host.cpp compiles the header that denoise.hip takes its weights, shares,
mix and limit from with g++ alone; every function is held to the CPU model (tests/denoise_model.py) on grids that include the
ends of every range.  The program is built twice, plainly and with -fsanitize=address,undefined (it has its own main): a sum or a
product that left its type, or a shift out of range, would be reported.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_L = 1020 * 25                                   # tolerance * n at their largest
MAX_W = (256 * MAX_L) >> 6                          # 102,000
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("denoise_on_host_" + request.param) / "denoise_on_host"
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "denoise_on_host.cpp"), "-o", str(out)])
    return out


def run(program, mode, rows):
    src, dst = program.parent / f"{mode}.in", program.parent / f"{mode}.out"
    np.ascontiguousarray(rows, np.uint32).tofile(src)
    subprocess.check_call([str(program), mode, str(src), str(dst)])
    return np.fromfile(dst, np.uint32).astype(np.int64)


def grid(*axes):
    return np.stack([a.reshape(-1) for a in np.meshgrid(*axes, indexing="ij")], -1)


def test_the_limits_are_the_headers(program):
    assert subprocess.check_output([str(program), "--limits"], text=True).split() == ["2", "2", "1020", "256", "255"]


def test_weights(program):
    """strength x L x cost around every edge: cost below, at and above L, both ends of each range, a target outside."""
    L = np.array([1, 2, 9, 32, 288, 800, 1020, 9180, MAX_L - 1, MAX_L])
    rows = grid(np.array([0, 1, 63, 64, 65, 192, 255, 256]), L, np.array([0, 1, 2, 8, 31, 32, 33, 287, 288, 1019, 1020, 9179, 9180, MAX_L - 1, MAX_L]),
                np.array([0, 1]))
    got = run(program, "weight", rows)
    want = dm.weight(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] != 0)
    assert (got == want).all()
    assert got.max() == MAX_W


def test_shares_on_a_grid_with_the_extremes(program):
    """Every (w_1, w_2, L) of a grid that holds the ends of each range and the values around powers of two, then 200,000 random
    reachable triples (w_i <= 4 L): the division equals the model's floor, the shares sum to 256 and curr keeps at least 1."""
    w = np.unique(np.concatenate([np.arange(0, 66), [127, 128, 255, 256, 257, 1000, 4079, 4080, 25500, 51000, 65535, 65536, MAX_W - 1, MAX_W]]))
    L = np.array([1, 2, 3, 9, 25, 32, 255, 256, 288, 800, 1020, 9180, MAX_L - 1, MAX_L])
    rng = np.random.default_rng(7)
    rl = rng.integers(1, MAX_L + 1, 200000)
    random = np.stack([rl, rng.integers(0, 4 * rl + 1), rng.integers(0, 4 * rl + 1)], -1)
    rows = np.concatenate([grid(L, w, w), random])
    got = run(program, "shares", rows).reshape(-1, 3)
    a0, a1, a2 = dm.shares(rows[:, 0], rows[:, 1], rows[:, 2])
    assert (got[:, 0] == a0).all() and (got[:, 1] == a1).all() and (got[:, 2] == a2).all()
    assert (got.sum(-1) == 256).all() and got[:, 0].min() >= 1
    assert (rows[:, 0] + rows[:, 1] + rows[:, 2]).max() == MAX_L + 2 * MAX_W          # D at its largest: 229,500


def texels(c, r1, r2):
    """Packed texels whose four channels hold four different arrangements of the bytes."""
    pack = lambda b: b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24)
    return pack([c, r1, 255 - c, c]), pack([r1, c, r1, 255 - r1]), pack([r2, 255 - r2, c, r1])


def unpack(px):
    return np.stack([(px >> k) & 255 for k in (0, 8, 16, 24)], -1)


def check_texels(program, a1, a2, limit):
    c, r1 = (v.reshape(-1) for v in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    r2 = (c * 7 + r1 * 13 + 5) % 256
    pc, p1, p2 = texels(c, r1, r2)
    rows = np.stack([np.full_like(c, a1), np.full_like(c, a2), np.full_like(c, limit), pc, p1, p2], -1)
    got = unpack(run(program, "texel", rows))
    cc, c1, c2 = unpack(pc), unpack(p1), unpack(p2)
    want = dm.mix(256 - a1 - a2, a1, a2, cc, c1, c2, limit)
    assert (got == want).all(), (a1, a2, limit)
    assert (np.abs(got - cc) <= limit).all()
    lo, hi = np.minimum(cc, np.minimum(c1, c2)), np.maximum(cc, np.maximum(c1, c2))
    if a2 == 0:
        lo, hi = np.minimum(cc, c1), np.maximum(cc, c1)
    assert ((got >= lo) & (got <= hi)).all()


@pytest.mark.parametrize("a1,a2", [(0, 0), (1, 0), (128, 0), (192, 0), (255, 0), (85, 85), (127, 128), (1, 254), (200, 55)])
def test_the_mix_on_all_byte_pairs(program, a1, a2):
    check_texels(program, a1, a2, 255)


@pytest.mark.parametrize("limit", [0, 1, 254, 255])
def test_the_limit(program, limit):
    check_texels(program, 192, 0, limit)
    check_texels(program, 100, 155, limit)
