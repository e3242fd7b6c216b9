"""lfg_host's --hole-reach where it needs no GPU: what the command line refuses, before a device context is made.  CPU only."""
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
    """The run ends with a message that names --hole-reach, a non-zero exit and no report; "Failed to initialize HIP" is what
    the first step that opens a device says when it fails, and what it would say here, where opening one takes a GPU."""
    p = subprocess.run([host_binary, *SMALL, *options], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and p.stdout == "" and "--hole-reach" in p.stderr, (options, p.returncode, p.stdout, p.stderr)
    assert "Failed to initialize HIP" not in p.stderr, p.stderr
    return p.stderr


@pytest.mark.parametrize("value", ["0", "-1", "256", "1000", "16px", ""])
def test_host_refuses_a_reach_outside_1_to_255(host_binary, value):
    assert "1 to 255" in refused(host_binary, "--interpolator", "compensated", "--hole-reach", value)


@pytest.mark.parametrize("options", [[], ["--interpolator", "shader"], ["--evaluate"]])
def test_host_refuses_a_reach_without_the_compensated_interpolator(host_binary, options):
    assert "--interpolator compensated" in refused(host_binary, "--hole-reach", "32", *options)


@pytest.mark.parametrize("options", [[], ["--evaluate"]])
def test_host_refuses_a_reach_for_extrapolated_frames(host_binary, options):
    err = refused(host_binary, "--hole-reach", "32", "--interpolator", "compensated", "--generation", "extrapolate", *options)
    assert "--generation extrapolate" in err


def test_help_names_the_option(host_binary):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--hole-reach N" in p.stdout + p.stderr
