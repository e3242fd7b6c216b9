"""csrc/lfg_record_plan.hpp without a GPU: tests/cpp/record_plan_check.cpp compiles the record kernels' launch plans -- the
division by a multiplier, the fixed grid and its refusal, the walk cursor, the histogram's row layout and rectangle, pair_match's
tiles, the 16-byte alignment rule and the split of a width -- with g++ alone (the header takes no ROCm include) and runs them as
loops over every workgroup, lane and trip: every item exactly once at 1, 2 and 256 CUs, nothing past the end, no workgroup beyond
what its 32-bit bins hold.  The kernels' constants are read from the .hip files, so the check walks what the kernels walk.  The
program is built twice, plainly and with -fsanitize=address,undefined (it has its own main).  CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linux-fg_amd", "csrc")
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
CONSTANTS = {"frame_diff.hip": ["kDiffThreads", "kDiffUnroll", "kDiffGroupsPerCu", "kDiffGroupPixels"],
             "frame_ssim.hip": ["kSsimWaves", "kSsimGroupsPerCu", "kSsimStripWindows", "kSsimSegmentRows", "kSsimGroupWindows"],
             "levels.hip": ["kHistThreads", "kHistUnroll", "kHistGroupsPerCu", "kHistGroupPixels"],
             "pair_stats.hip": ["kPairBlockX", "kPairBlockY", "kPairUnroll", "kPairGroupsPerCu"]}


def kernel_constants():
    """-DK_DIFF_THREADS=1024 ... "-DK_DIFF_GROUP_PIXELS=(1ull << 31)" from `constexpr int kDiffThreads = 1024;`,
    `constexpr unsigned long long kDiffGroupPixels = 1ull << 31;` and `constexpr int kPairBlockX = 64, kPairBlockY = 4;` in the
    kernels' files."""
    out = []
    for name, constants in CONSTANTS.items():
        text = open(os.path.join(CSRC, name)).read()
        for c in constants:
            value = re.search(r"constexpr (?:int|unsigned long long) (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % c, text).group(1)
            out.append("-DK_" + re.sub(r"(?<!^)([A-Z])", r"_\1", c[1:]).upper() + "=(" + value + ")")
    return out


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("record_plan_check_" + request.param) / "record_plan_check"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", *kernel_constants(), "-I", CSRC,
               os.path.join(ROOT, "tests", "cpp", "record_plan_check.cpp"), "-o", str(out)]
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(command)
    return out


def test_record_plans_keep_their_contract(program):
    p = subprocess.run([str(program)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.startswith("ok "), p.stdout


def test_the_header_takes_no_rocm_include():
    text = open(os.path.join(CSRC, "lfg_record_plan.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
