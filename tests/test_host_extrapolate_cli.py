"""lfg_host's --generation where it needs no GPU: what the command line refuses, before a device context is made.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linux-fg_amd", "lfg_host")
SMALL = ["--input-width", "64", "--input-height", "36", "--frames", "3", "--quiet"]


@pytest.fixture(scope="module")
def host_binary():
    if not os.path.exists(HOST):
        import __graft_entry__ as entry
        entry.build()
    return HOST


def refused(host_binary, *options):
    """The run ends with a message that names --generation, a non-zero exit and no report; "Failed to initialize HIP" is what
    the first step that opens a device says when it fails, and what it would say here, where opening one takes a GPU."""
    p = subprocess.run([host_binary, *SMALL, *options], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and p.stdout == "" and "--generation" in p.stderr, (options, p.returncode, p.stdout, p.stderr)
    assert "Failed to initialize HIP" not in p.stderr, p.stderr
    return p.stderr


def test_host_refuses_an_unknown_generation(host_binary):
    assert "interpolate|extrapolate" in refused(host_binary, "--generation", "bogus", "--interpolator", "compensated")


@pytest.mark.parametrize("options", [[], ["--interpolator", "shader"], ["--evaluate"]])
def test_host_refuses_extrapolation_without_the_compensated_interpolator(host_binary, options):
    assert "--interpolator compensated" in refused(host_binary, "--generation", "extrapolate", *options)


def test_host_refuses_extrapolation_in_batch_mode(host_binary, tmp_path):
    err = refused(host_binary, "--generation", "extrapolate", "--interpolator", "compensated", "--ranks", "2", "--rank", "0",
                  "--comm-file", str(tmp_path / "id"), "--comm-nonce", "7")
    assert "--ranks" in err


def test_help_names_the_option(host_binary):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--generation interpolate|extrapolate" in p.stdout + p.stderr
