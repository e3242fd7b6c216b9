"""lfg_host's command line where it needs no GPU: what it refuses, before a device context is made, through the real binary.
CPU only.  (--hole-reach and --scale-filter keep files of their own, test_host_fill_cli.py and test_host_resample_cli.py; what the
command line accepts, and its report line: test_host_options.py.)"""
import subprocess

import pytest

from tests.host_cli import LENIENT, NAMES, TEXT, WHOLE, host_binary, refused  # noqa: F401  (host_binary is a fixture)

COMPENSATED = ["--interpolator", "compensated"]
BATCH = ["--ranks", "2", "--rank", "0", "--comm-file", "unused", "--comm-nonce", "7"]

# ---- everything parsing refuses: the whole message, exit code 1 -----------------------------------------------------------
PARSE = ([([name, bad], f"Invalid {name} ({hint})") for name, lo, hi, hint in WHOLE for bad in (str(lo - 1), str(hi + 1), "1x", "0.5", "")]
         + [([name, bad], f"Invalid {name} ({names})") for name, names in NAMES for bad in ("bogus", names.split("|")[0] + " ", "")]
         + [(["--factors", bad], "Invalid --factors list") for bad in ("x", "0.25,,0.5", "0.5;0.75")]
         + [([bad], "Invalid stream index") for bad in ("1x", "0.5", "--no-such-option")]
         # an option that needs a value and stands last is read as the stream index
         + [([name], "Invalid stream index") for name in [w[0] for w in WHOLE] + [n[0] for n in NAMES] + LENIENT + TEXT])


@pytest.mark.parametrize("options,message", PARSE, ids=lambda a: "_".join(a).replace("--", "") if isinstance(a, list) else None)
def test_host_refuses_what_does_not_parse(host_binary, options, message):
    refused(host_binary, message, *options, code=1)


# ---- every rule of what cannot be combined, in the order the rules are tried: the whole message, exit code 2 -----------------
NV12_IN = ["--input-format", "nv12", "--input-raw", "unused"]
SUBPEL = ["--subpel-vectors", "1", *COMPENSATED]
CLASH = [
    ([*NV12_IN, *BATCH], "--input-format nv12 cannot be combined with --ranks"),
    (["--output-format", "nv12", "--evaluate"], "--output-format nv12 cannot be combined with --evaluate"),
    (["--input-format", "nv12"], "--input-format nv12 needs --input-raw (the synthetic source makes RGBA8)"),
    ([*NV12_IN, "--input-width", "63"], "NV12 needs an even width and height"),
    (["--output-format", "nv12", "--output-width", "128", "--output-height", "71"], "NV12 needs an even width and height"),
    (["--scale-filter", "lanczos3", "--output-width", "5", "--output-height", "4"], "--scale-filter lanczos3 cannot scale 64 to 5 (more than 64 taps per sample)"),
    (["--scale-filter", "bilinear", "--output-width", "2", "--output-height", "1"], "--scale-filter bilinear cannot scale 36 to 1 (more than 64 taps per sample)"),
    (["--generation", "extrapolate"], "--generation extrapolate needs --interpolator compensated"),
    (["--generation", "extrapolate", *COMPENSATED, *BATCH], "--generation extrapolate cannot be combined with --ranks"),
    (["--hole-reach", "32"], "--hole-reach needs --interpolator compensated"),
    (["--hole-reach", "32", *COMPENSATED, "--generation", "extrapolate"], "--hole-reach cannot be combined with --generation extrapolate"),
    (["--subpel-vectors", "1"], "--subpel-vectors cannot be combined with --interpolator shader"),
    ([*SUBPEL, "--generation", "extrapolate"], "--subpel-vectors cannot be combined with --generation extrapolate"),
    ([*SUBPEL, "--bidirectional", "0"], "--subpel-vectors cannot be combined with --bidirectional"),
    ([*SUBPEL, "--protect-static", "0"], "--subpel-vectors cannot be combined with --protect-static"),
    ([*SUBPEL, "--hole-reach", "1"], "--subpel-vectors cannot be combined with --hole-reach"),
    ([*SUBPEL, *BATCH], "--subpel-vectors cannot be combined with --ranks"),
    (["--evaluate", *BATCH], "--evaluate cannot be combined with --ranks"),
    (["--evaluate", "--factors", "0.25,0.5"], "--evaluate cannot be combined with --factors"),
    (["--evaluate", "--no-interpolation"], "--evaluate cannot be combined with --no-interpolation"),
    (["--evaluate", "--output-raw", "unused"], "--evaluate cannot be combined with --output-raw"),
    (["--evaluate", "--dump-dir", "unused"], "--evaluate cannot be combined with --dump-dir"),
    (["--evaluate", "--replay", "2"], "--evaluate cannot be combined with --replay"),
    (["--evaluate", "--frames", "2"], "--evaluate needs --frames of 3 or more"),
    # two faults: the rule tried first names its own
    ([*NV12_IN, "--input-width", "63", "--scale-filter", "lanczos3", "--output-width", "5"], "NV12 needs an even width and height"),
    (["--scale-filter", "lanczos3", "--output-width", "5", "--generation", "extrapolate"], "--scale-filter lanczos3 cannot scale 64 to 5 (more than 64 taps per sample)"),
    (["--generation", "extrapolate", "--hole-reach", "32", "--subpel-vectors", "1"], "--generation extrapolate needs --interpolator compensated"),
    (["--hole-reach", "32", "--subpel-vectors", "1", "--evaluate", "--replay", "2"], "--hole-reach needs --interpolator compensated"),
    ([*SUBPEL, "--bidirectional", "0", "--protect-static", "0", "--evaluate", *BATCH], "--subpel-vectors cannot be combined with --bidirectional"),
]


@pytest.mark.parametrize("options,message", CLASH, ids=[f"{i}_{m.split(' ')[0].lstrip('-')}" for i, (_, m) in enumerate(CLASH)])
def test_host_refuses_what_cannot_be_combined(host_binary, options, message):
    refused(host_binary, message, *options, code=2)


# ---- the cases of six options' own test files, as they were --------------------------------------------------------------
RANGES = [("--bidirectional", COMPENSATED, ["-2", "65", "1020", "12x", "", "0.5"]),
          ("--half-res-motion", ["--motion", "pyramid"], ["-2", "3", "one", "1x", "", "0.5"]),
          ("--protect-static", COMPENSATED, ["-2", "1021", "12x", "", "0.5"]),
          ("--sharpen", [], ["-1", "65", "1x", "", "0.5"])]


@pytest.mark.parametrize("option,before,value", [pytest.param(o, b, v, id=f"{o[2:]}_{v}") for o, b, values in RANGES for v in values])
def test_host_refuses_a_value_out_of_range(host_binary, option, before, value):
    refused(host_binary, option, *before, option, value)


def test_host_refuses_an_unknown_generation(host_binary):
    assert "interpolate|extrapolate" in refused(host_binary, "--generation", "--generation", "bogus", *COMPENSATED)


@pytest.mark.parametrize("options", [[], ["--interpolator", "shader"], ["--evaluate"]])
def test_host_refuses_extrapolation_without_the_compensated_interpolator(host_binary, options):
    assert "--interpolator compensated" in refused(host_binary, "--generation", "--generation", "extrapolate", *options)


def test_host_refuses_extrapolation_in_batch_mode(host_binary, tmp_path):
    err = refused(host_binary, "--generation", "--generation", "extrapolate", *COMPENSATED, "--ranks", "2", "--rank", "0",
                  "--comm-file", str(tmp_path / "id"), "--comm-nonce", "7")
    assert "--ranks" in err


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
    refused(host_binary, word, *args)


@pytest.mark.parametrize("words", [["--bidirectional T"], ["--half-res-motion R"], ["--generation interpolate|extrapolate"],
                                   ["--protect-static T"], ["--sharpen S"]], ids=lambda w: w[0][2:])
def test_help_names_the_option(host_binary, words):
    p = subprocess.run([host_binary, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and all(word in p.stdout + p.stderr for word in words)
