"""lfg_host's --scale-filter where it needs no GPU: what the command line refuses, before a device context is made.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linux-fg_amd", "lfg_host")
SIZE = ["--input-width", "64", "--input-height", "36", "--frames", "2", "--quiet"]


@pytest.fixture(scope="module")
def host_binary():
    if not os.path.exists(HOST):
        import __graft_entry__ as entry
        entry.build()
    return HOST


@pytest.mark.parametrize("value", ["", "lanczos", "Lanczos3", "bicubic", "5", "catmull_rom", "lanczos3 "])
def test_host_refuses_an_unknown_filter(host_binary, value):
    p = subprocess.run([host_binary, *SIZE, "--scale-filter", value], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and p.stdout == "" and "--scale-filter" in p.stderr, (value, p.returncode, p.stdout, p.stderr)


@pytest.mark.parametrize("name,width,height,refused", [("lanczos3", 6, 4, False), ("lanczos3", 5, 4, True), ("lanczos3", 6, 3, True),
                                                       ("bilinear", 2, 2, False), ("bilinear", 1, 2, True)])
def test_host_refuses_a_ratio_past_the_tap_limit(host_binary, name, width, height, refused):
    """64 x 36 to width x height: 64 -> 6 is 10.67 : 1, Lanczos-3's 64 taps exactly; 64 -> 5 and 36 -> 3 are past it; the
    triangle has 64 taps at 32 : 1.  A ratio within the limit goes on to look for a device, whatever it finds."""
    p = subprocess.run([host_binary, *SIZE, "--scale-filter", name, "--output-width", str(width), "--output-height", str(height)],
                       capture_output=True, text=True, timeout=60)
    if refused:
        assert p.returncode == 2 and p.stdout == "" and "64 taps" in p.stderr, (p.returncode, p.stdout, p.stderr)
    else:
        assert "64 taps" not in p.stderr and "--scale-filter" not in p.stderr, p.stderr


def test_help_names_the_option_and_every_filter(host_binary):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    text = p.stdout + p.stderr
    assert p.returncode == 0 and "--scale-filter F" in text
    assert all(name in text for name in ("reference", "nearest", "bilinear", "catmull-rom", "mitchell", "lanczos2", "lanczos3"))
