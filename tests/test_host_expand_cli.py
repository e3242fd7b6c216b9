"""lfg_host's --half-res-motion where it needs no GPU: what the command line refuses, before a device context is made.  CPU only."""
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


@pytest.mark.parametrize("value", ["-2", "3", "one", "1x", "", "0.5"])
def test_host_refuses_a_radius_out_of_range(host_binary, value):
    p = subprocess.run([host_binary, "--input-width", "64", "--input-height", "36", "--frames", "2", "--quiet",
                        "--motion", "pyramid", "--half-res-motion", value], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and p.stdout == "" and "--half-res-motion" in p.stderr, (value, p.returncode, p.stdout, p.stderr)
    assert "Failed to initialize HIP" not in p.stderr, p.stderr       # refused before a device is opened


def test_help_names_the_option(host_binary):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--half-res-motion R" in p.stdout + p.stderr
