"""lfg_host's --scale-filter where it needs no GPU: what the command line refuses, before a device context is made.  CPU only."""
import subprocess

import pytest

from tests.host_cli import SMALL, host_binary, refused  # noqa: F401  (host_binary is a fixture)


@pytest.mark.parametrize("value", ["", "lanczos", "Lanczos3", "bicubic", "5", "catmull_rom", "lanczos3 "])
def test_host_refuses_an_unknown_filter(host_binary, value):
    refused(host_binary, "--scale-filter", "--scale-filter", value)


@pytest.mark.parametrize("name,width,height,refuses", [("lanczos3", 6, 4, False), ("lanczos3", 5, 4, True), ("lanczos3", 6, 3, True),
                                                       ("bilinear", 2, 2, False), ("bilinear", 1, 2, True)])
def test_host_refuses_a_ratio_past_the_tap_limit(host_binary, name, width, height, refuses):
    """64 x 36 to width x height: 64 -> 6 is 10.67 : 1, Lanczos-3's 64 taps exactly; 64 -> 5 and 36 -> 3 are past it; the
    triangle has 64 taps at 32 : 1.  A ratio within the limit goes on to look for a device, whatever it finds."""
    p = subprocess.run([host_binary, *SMALL, "--scale-filter", name, "--output-width", str(width), "--output-height", str(height)],
                       capture_output=True, text=True, timeout=60)
    if refuses:
        assert p.returncode == 2 and p.stdout == "" and "64 taps" in p.stderr, (p.returncode, p.stdout, p.stderr)
    else:
        assert "64 taps" not in p.stderr and "--scale-filter" not in p.stderr, p.stderr


def test_help_names_the_option_and_every_filter(host_binary):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    text = p.stdout + p.stderr
    assert p.returncode == 0 and "--scale-filter F" in text
    assert all(name in text for name in ("reference", "nearest", "bilinear", "catmull-rom", "mitchell", "lanczos2", "lanczos3"))
