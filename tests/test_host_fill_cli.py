"""lfg_host's --hole-reach where it needs no GPU: what the command line refuses, before a device context is made.  CPU only."""
import subprocess

import pytest

from tests.host_cli import host_binary, refused  # noqa: F401  (host_binary is a fixture)


@pytest.mark.parametrize("value", ["0", "-1", "256", "1000", "16px", ""])
def test_host_refuses_a_reach_outside_1_to_255(host_binary, value):
    assert "1 to 255" in refused(host_binary, "--hole-reach", "--interpolator", "compensated", "--hole-reach", value)


@pytest.mark.parametrize("options", [[], ["--interpolator", "shader"], ["--evaluate"]])
def test_host_refuses_a_reach_without_the_compensated_interpolator(host_binary, options):
    assert "--interpolator compensated" in refused(host_binary, "--hole-reach", "--hole-reach", "32", *options)


@pytest.mark.parametrize("options", [[], ["--evaluate"]])
def test_host_refuses_a_reach_for_extrapolated_frames(host_binary, options):
    err = refused(host_binary, "--hole-reach", "--hole-reach", "32", "--interpolator", "compensated", "--generation", "extrapolate", *options)
    assert "--generation extrapolate" in err


def test_help_names_the_option(host_binary):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--hole-reach N" in p.stdout + p.stderr
