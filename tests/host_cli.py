"""lfg_host for the tests: the one place that finds or builds it, and that starts it for what the command line refuses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linux-fg_amd", "lfg_host")
SMALL = ["--input-width", "64", "--input-height", "36", "--frames", "3", "--quiet"]

# lfg_host's options by how their value is read: a whole number in [lo, hi] with the hint of its message; one of a list of names;
# atoi of whatever stands there; text the option reads itself; and the flags, which take none.  A new option is one row here.
WHOLE = [("--refine-vectors", -1, 2, "-1, 0, 1 or 2"), ("--cut-threshold", -1, 1000, "-1, or 0 to 1000"),
         ("--protect-static", -1, 1020, "-1, or 0 to 1020"), ("--bidirectional", -1, 64, "-1, or 0 to 64"),
         ("--half-res-motion", -1, 2, "-1, 0, 1 or 2"), ("--hole-reach", 1, 255, "1 to 255"),
         ("--subpel-vectors", -1, 2, "-1, 0, 1 or 2"), ("--sharpen", 0, 64, "0 to 64")]
NAMES = [("--motion", "full|pyramid"), ("--semantics", "reference|intended"), ("--interpolator", "shader|compensated"),
         ("--generation", "interpolate|extrapolate"), ("--input-format", "rgba|nv12"), ("--output-format", "rgba|nv12"),
         ("--yuv-matrix", "601|709"), ("--yuv-range", "limited|full"), ("--chroma", "replicate|left"),
         ("--scale-filter", "reference|nearest|bilinear|catmull-rom|mitchell|lanczos2|lanczos3")]
LENIENT = ["--input-width", "--input-height", "--output-width", "--output-height", "--target-fps", "--in-flight", "--ranks", "--rank",
           "--frames", "--device", "--replay"]
TEXT = ["--interpolation-factor", "--factors", "--comm-file", "--comm-nonce", "--dump-dir", "--input-raw", "--output-raw"]
FLAGS = ["--help", "--no-interpolation", "--evaluate", "--sync-present", "--present-null", "--quiet"]


def built(path=HOST):
    """`path`, after a build if nothing is there."""
    if not os.path.exists(path):
        import __graft_entry__ as entry
        entry.build()
    return path


@pytest.fixture(scope="module")
def host_binary():
    return built()


def refused(host_binary, word, *options, code=None):
    """The run ends with a message that has `word` in it, a non-zero exit and no report; "Failed to initialize HIP" is what the
    first step that opens a device says when it fails, and what it would say here, where opening one takes a GPU.  With `code`:
    that exit code, and `word` is the whole of the one line logged."""
    p = subprocess.run([host_binary, *SMALL, *options], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and p.stdout == "" and word in p.stderr, (options, p.returncode, p.stdout, p.stderr)
    assert "Failed to initialize HIP" not in p.stderr, p.stderr
    if code is not None:
        assert p.returncode == code and p.stderr.split(" ERROR   ", 1)[1:] == [word + "\n"], (options, p.returncode, p.stderr)
    return p.stderr
