"""lfg_host's NV12 options where they need no GPU: what the command line refuses, before a device context is made.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linux-fg_amd", "lfg_host")


@pytest.fixture(scope="module")
def host_binary():
    if not os.path.exists(HOST):
        import __graft_entry__ as entry
        entry.build()
    return HOST


@pytest.mark.parametrize("args,word", [
    (["--input-format", "nv12"], "--input-raw"),                                                # the synthetic source makes RGBA8
    (["--input-format", "nv12", "--input-raw", "unused", "--input-width", "63"], "even"),
    (["--input-format", "nv12", "--input-raw", "unused", "--input-height", "35"], "even"),
    (["--output-format", "nv12", "--output-width", "127", "--output-height", "72"], "even"),
    (["--output-format", "nv12", "--evaluate", "--frames", "3"], "--evaluate"),
    (["--input-format", "nv12", "--input-raw", "unused", "--ranks", "1", "--rank", "0", "--comm-file", "unused"], "--ranks"),
    (["--input-format", "yuy2"], "rgba|nv12"), (["--output-format", "i420"], "rgba|nv12"),
    (["--yuv-matrix", "2020"], "601|709"), (["--yuv-range", "wide"], "limited|full"), (["--chroma", "centre"], "replicate|left"),
], ids=lambda a: "_".join(a).replace("--", "") if isinstance(a, list) else None)
def test_host_refuses_what_nv12_cannot_do(host_binary, args, word):
    p = subprocess.run([host_binary, "--input-width", "64", "--input-height", "36", "--frames", "2", "--quiet", *args],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and p.stdout == "" and word in p.stderr, (args, p.returncode, p.stdout, p.stderr)
