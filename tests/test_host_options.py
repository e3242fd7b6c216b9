"""host/options.cpp on its own (tests/cpp/host_options_check.cpp, g++ alone): what lfg_host's command line accepts and where each
value lands, the report line against its former form, and the option table against the usage text.  CPU only.
(What the command line refuses, through the real binary: test_host_cli.py.)"""
import json
import os
import subprocess

import pytest

from tests.host_cli import FLAGS, LENIENT, NAMES, ROOT, TEXT, WHOLE

DEFAULTS = dict(inputWidth=1920, inputHeight=1080, outputWidth=1920, outputHeight=1080, targetFps=60, enableInterpolation=1,
                interpolationFactor=0.5, sharpen=0, scaleFilter=-1, estimator=0, semantics=0, interpolator=0, generation=0, refineRadius=-1,
                cutThreshold=-1, staticTolerance=-1, bidirectional=-1, halfResMotion=-1, holeReach=-1, subpelVectors=-1, inputNv12=0,
                outputNv12=0, yuvMatrix=1, yuvRange=0, yuvSiting=1, factors=[], inFlight=2, ranks=0, rank=0, commFile="", commNonce=0,
                frames=10, device=0, replay=0, stream=0, dumpDir="", inputRaw="", outputRaw="", help=0, quiet=0, evaluate=0,
                syncPresent=0, presentNull=0)
FIELD = {"--refine-vectors": "refineRadius", "--cut-threshold": "cutThreshold", "--protect-static": "staticTolerance",
         "--bidirectional": "bidirectional", "--half-res-motion": "halfResMotion", "--hole-reach": "holeReach",
         "--subpel-vectors": "subpelVectors", "--sharpen": "sharpen", "--motion": "estimator", "--semantics": "semantics",
         "--interpolator": "interpolator", "--generation": "generation", "--input-format": "inputNv12", "--output-format": "outputNv12",
         "--yuv-matrix": "yuvMatrix", "--yuv-range": "yuvRange", "--chroma": "yuvSiting", "--scale-filter": "scaleFilter"}
SIZE = ["--input-width", "64", "--input-height", "36"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "host_options_check"
    host = os.path.join(ROOT, "linux-fg_amd", "host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_options_check.cpp"), os.path.join(host, "options.cpp"), "-o", str(out)])
    return str(out)


ACCEPTED = (
    [([], {})]
    # both ends of every range, every name of every list (the constants of include/linuxfg_hip.h count from 0; reference is -1)
    + [([name, str(v)], {FIELD[name]: v}) for name, lo, hi, _ in WHOLE for v in (lo, hi)]
    + [([name, word], {FIELD[name]: i - (name == "--scale-filter")}) for name, names in NAMES for i, word in enumerate(names.split("|"))]
    # the last occurrence wins
    + [(["--hole-reach", "3", "--hole-reach", "200"], {"holeReach": 200}), (["--motion", "pyramid", "--motion", "full"], {"estimator": 0}),
       (["--scale-filter", "mitchell", "--scale-filter", "reference"], {"scaleFilter": -1}), (["--frames", "4", "--frames", "6"], {"frames": 6}),
       (["--factors", "0.5", "--factors", "0.25,0.5,0.75"], {"factors": [0.25, 0.5, 0.75]}), (["3", "5"], {"stream": 5})]
    # the output size: both sides, the height alone, the width alone (truncated), neither
    + [([*SIZE, "--output-width", "100", "--output-height", "50"], {"inputWidth": 64, "inputHeight": 36, "outputWidth": 100, "outputHeight": 50}),
       ([*SIZE, "--output-height", "72"], {"inputWidth": 64, "inputHeight": 36, "outputWidth": 128, "outputHeight": 72}),
       ([*SIZE, "--output-width", "100"], {"inputWidth": 64, "inputHeight": 36, "outputWidth": 100, "outputHeight": 56}),
       (SIZE, {"inputWidth": 64, "inputHeight": 36, "outputWidth": 64, "outputHeight": 36}),
       (["--output-height", "2160"], {"outputWidth": 3840, "outputHeight": 2160})]
    # atoi's leniency, the text options, the flags, the stream index
    + [(["--frames", "12abc", "--replay", "x", "--device", "-1", "--in-flight", " 3", "--target-fps", "144"],
        {"frames": 12, "replay": 0, "device": -1, "inFlight": 3, "targetFps": 144}),
       (["--ranks", "2", "--rank", "1", "--comm-file", "id", "--comm-nonce", "0x10"], {"ranks": 2, "rank": 1, "commFile": "id", "commNonce": 16}),
       (["--interpolation-factor", "0.25", "--dump-dir", "d", "--input-raw", "-", "--output-raw", "o"],
        {"interpolationFactor": 0.25, "dumpDir": "d", "inputRaw": "-", "outputRaw": "o"}),
       (["--no-interpolation", "--evaluate", "--sync-present", "--present-null", "--quiet", "0x11"],
        {"enableInterpolation": 0, "evaluate": 1, "syncPresent": 1, "presentNull": 1, "quiet": 1, "stream": 17}),
       (["--frames", "5", "--help", "--frames", "bogus", "--sharpen", "99"], {"frames": 5, "help": 1, "inputWidth": 0, "inputHeight": 0,
                                                                               "outputWidth": 0, "outputHeight": 0})])


@pytest.mark.parametrize("args,changed", ACCEPTED, ids=lambda a: "_".join(a).replace("--", "") if isinstance(a, list) else None)
def test_options_land_where_they_belong(check, args, changed):
    env = {k: v for k, v in os.environ.items() if k != "LFG_COMM_NONCE"}
    p = subprocess.run([check, "parse", *args], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout
    assert json.loads(p.stdout) == {**DEFAULTS, **changed}


@pytest.mark.parametrize("args,nonce", [([], 77), (["--comm-nonce", "5"], 5), (["--comm-nonce", "0"], 0)])
def test_comm_nonce_comes_from_the_environment_unless_given(check, args, nonce):
    p = subprocess.run([check, "parse", *args], capture_output=True, text=True, env={**os.environ, "LFG_COMM_NONCE": "77"})
    assert p.returncode == 0 and json.loads(p.stdout) == {**DEFAULTS, "commNonce": nonce}, p.stdout


@pytest.mark.parametrize("args,message", [
    ([], ""), ([*SIZE, "--scale-filter", "bilinear", "--output-width", "8", "--output-height", "36"], ""),
    ([*SIZE, "--scale-filter", "bilinear", "--output-width", "7", "--output-height", "36"], "--scale-filter bilinear cannot scale 64 to 7 (more than 64 taps per sample)"),
    ([*SIZE, "--scale-filter", "lanczos3", "--output-width", "8", "--output-height", "4"], "--scale-filter lanczos3 cannot scale 36 to 4 (more than 64 taps per sample)"),
    ([*SIZE, "--scale-filter", "reference", "--output-width", "1", "--output-height", "1"], ""),          # lfg_scale: no tap limit asked
    ([*SIZE, "--output-format", "nv12", "--output-width", "7", "--scale-filter", "nearest"], "NV12 needs an even width and height"),
    ([*SIZE, "--scale-filter", "nearest", "--output-width", "7", "--hole-reach", "9"], "--scale-filter nearest cannot scale 64 to 7 (more than 64 taps per sample)"),
    ([*SIZE, "--scale-filter", "nearest", "--output-width", "8", "--output-height", "36", "--hole-reach", "9"], "--hole-reach needs --interpolator compensated"),
], ids=lambda a: "_".join(a).replace("--", "") if isinstance(a, list) else None)
def test_check_asks_the_callers_tap_limit_in_its_place(check, args, message):
    """The check program hands CheckOptions a tap limit of its own, which every ratio up to 8 : 1 meets whatever the filter: the
    verdict is the caller's, both axes are asked, width first, after the NV12 rules and before the route's."""
    p = subprocess.run([check, "check", *args], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == message + "\n", p.stdout


def test_report_line_equals_its_former_form(check):
    """729 settings of the six optional fields (each absent, least, greatest) x 128: both branches, both formats at both doors,
    replay 0 and 8, --sync-present, --present-null, small and large counters."""
    p = subprocess.run([check, "report"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == f"ok {729 * 128}\n", p.stdout[-2000:]


def test_usage_text_and_option_table_name_the_same_options(check):
    p = subprocess.run([check, "usage"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout
    rows, mentions = map(int, p.stdout.split()[1:])
    assert rows == len(WHOLE) + len(NAMES) + len(LENIENT) + len(TEXT) + len(FLAGS) and mentions >= rows
