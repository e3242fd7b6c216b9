"""oracle/glsl_shim.hpp held to known answers: tests/cpp/glsl_shim_check.cpp is compiled with g++ alone and run twice, plainly
and with -fsanitize=address,undefined (it has its own main; nothing of it is loaded into python).  The known answers are the
built-ins where a slip would go unnoticed because the oracle could share it: float -> int truncation, fract of a negative,
texelFetch outside the image, the UNORM store's ties, clamps and NaN, texture at exact centres and at uv 0 and 1, the
summation order of distance, and mix.  Where oracle/_ref/ holds the generated shader sources they are linked in, and each
shader also runs on a tiny image under the sanitizers.  CPU only."""
import os
import subprocess

import pytest

import oracle
from oracle import ref_recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"plain": ["-O1"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def ref_sources():
    if not oracle.ref_available():
        return []
    paths = [os.path.join(ref_recipe.REF_DIR, n + ".cpp") for n in ref_recipe.SHADERS]
    return paths if all(os.path.exists(p) for p in paths) else []


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("glsl_shim_check_" + request.param) / "glsl_shim_check"
    shaders = ref_sources()
    command = ["g++", *FLAGS[request.param], "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fno-fast-math",
               "-I", os.path.join(ROOT, "oracle"), *(["-DLFG_HAVE_REF_SHADERS"] if shaders else []),
               os.path.join(ROOT, "tests", "cpp", "glsl_shim_check.cpp"), *shaders, "-o", str(out), "-lpthread"]
    if request.param == "sanitized":
        probe = out.parent / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(out.parent / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no ASan / UBSan runtimes")
    subprocess.check_call(command)
    return out, bool(shaders)


def test_the_shim_gives_the_known_answers(program):
    binary, with_shaders = program
    p = subprocess.run([str(binary)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.startswith("ok "), p.stdout
    print(p.stdout.strip(), "with the three shaders" if with_shaders else "without shader sources")


def test_the_shim_takes_the_standard_library_only():
    text = open(os.path.join(ROOT, "oracle", "glsl_shim.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<c") for i in includes), includes
