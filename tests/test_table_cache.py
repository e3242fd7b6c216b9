"""csrc/lfg_table_cache.hpp without a GPU: tests/cpp/table_cache_check.cpp compiles the C-ABI layer's upload, bounded table cache
and grow-only lane buffer with g++ alone (the header takes no ROCm include) and holds them to their contract on a fake device
that counts allocations, frees, copies and outstanding blocks and fails the n-th of them on request.  The program is built
twice, plainly and with -fsanitize=address,undefined (it has its own main): a table freed while a call holds it, or freed
twice, is then a report as well as a failed check.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("table_cache_check_" + request.param) / "table_cache_check"
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "linux-fg_amd", "csrc"),
               os.path.join(ROOT, "tests", "cpp", "table_cache_check.cpp"), "-o", str(out)]
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(command)
    return out


def test_table_cache_and_lane_buffer_keep_their_contract(program):
    p = subprocess.run([str(program)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.startswith("ok "), p.stdout


def test_the_header_takes_no_rocm_include():
    text = open(os.path.join(ROOT, "linux-fg_amd", "csrc", "lfg_table_cache.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
