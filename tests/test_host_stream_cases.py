"""The cases of tests/host_stream_cases.py can fail: on the small stream the expected frames tell a stale or swapped slot, every
option of the all-on rows shows, the cuts fall where the stream puts them, and the order and the counts are the ones
stated here by hand.  CPU only: the models of tests/ and the oracle."""
import numpy as np
import pytest

from tests import host_stream_cases as hc

W, H, N = hc.SMALL
CUTS = [0, 2, 3, 4]                                  # of the pairs (0, 1) .. (4, 5): the first, two in the middle, the last
ROW_IDS = [r["name"] for r in hc.ROWS]


@pytest.fixture(scope="module")
def frames(oracle):
    return hc.stream(W, H, N)


@pytest.fixture(scope="module")
def expected(frames):
    return {r["name"]: hc.expected_cpu(frames, r) for r in hc.ROWS}


def packed(frame):
    return b"".join(np.ascontiguousarray(part).tobytes() for part in (frame if isinstance(frame, tuple) else (frame,)))


def test_the_stream_is_what_its_docstring_says(frames):
    assert len(frames) == N and all(f.shape == (H, W, 4) and f.dtype == np.uint8 for f in frames)
    assert len({f.tobytes() for f in frames}) == N
    assert list(hc.cut_pairs(N)) == CUTS and list(hc.cut_pairs(12)) == [0, 5, 6, 10]
    on, px = hc.overlay(W, H)
    assert 150 < on.sum() < 400 and all((f[on] == px[on]).all() for f in frames)
    big = hc.stream(640, 360, 12)
    assert len({f.tobytes() for f in big}) == 12 and all(f.shape == (360, 640, 4) for f in big)


@pytest.mark.parametrize("name", ROW_IDS)
def test_cuts_fall_where_the_stream_puts_them(frames, name):
    """With detection on (rows A to C, E and F have it; rows D and G are measured as if they had), exactly the four cut pairs fall below the
    threshold, and every pair keeps ROOM pixels per thousand between itself and the threshold."""
    e = hc.expected_cpu(frames, dict(hc.ROW[name], threshold=hc.THRESHOLD))
    print(f"row {name}: matched per thousand {e['permille']}")
    assert e["cut_at"] == CUTS and e["cuts"] == 4
    for k, p in enumerate(e["permille"]):
        assert (p <= hc.THRESHOLD - hc.ROOM) if k in CUTS else (p >= hc.THRESHOLD + hc.ROOM), (k, p)


def test_order_counts_and_cuts_are_the_hand_stated_ones(expected):
    g, r = True, False
    assert expected["A"]["flags"] == [r] + [g, g, g, r] * 5                 # generated frames, then the real one
    assert expected["B"]["flags"] == [r] + [r, g, g] * 5                    # extrapolating: the real one first
    assert expected["C"]["flags"] == expected["D"]["flags"] == expected["G"]["flags"] == [r] + [g, r] * 5
    assert expected["E"]["flags"] == expected["A"]["flags"] and expected["F"]["flags"] == [r] + [g, g, r] * 5
    counts = {name: (e["presented"], e["interpolated"], e["cuts"], e["cut_at"]) for name, e in expected.items()}
    assert counts == {"A": (21, 15, 4, CUTS), "B": (16, 10, 4, CUTS), "C": (11, 5, 4, CUTS), "D": (11, 5, 0, []),
                      "E": (21, 15, 4, CUTS), "F": (16, 10, 4, CUTS), "G": (11, 5, 0, [])}
    for r_ in hc.ROWS:
        e = expected[r_["name"]]
        fields = hc.report_fields(r_, N)
        assert (fields["presented"], fields["interpolated"]) == (e["presented"], e["interpolated"])
        assert all(isinstance(f, tuple) == r_["nv12_out"] for f in e["frames"])
    # a one-lane run of the small stream reuses no read-back slot with three factors; the schedules' stream of 12 frames does
    assert hc.readback_slots(3, hc.ROW["A"]) == 18 and hc.readback_slots(3, hc.ROW["C"]) == 10 and hc.readback_slots(1, hc.ROW["B"]) == 8
    assert hc.report_fields(hc.ROW["A"], 12)["presented"] == 45 and hc.report_fields(hc.ROW["D"], 12)["presented"] == 23
    assert hc.readback_slots(3, hc.ROW["E"]) == 18 and hc.readback_slots(3, hc.ROW["F"]) == 14 and hc.readback_slots(3, hc.ROW["G"]) == 10
    assert [hc.report_fields(hc.ROW[n], 12)["presented"] for n in "EFG"] == [45, 34, 23]


def test_a_cut_shows_source_frames(frames, expected):
    """Across a cut the generated frames are source frames: prev below 0.5 and curr from 0.5 on, always curr when extrapolating.
    Row C's frames are RGBA and sharpened, so they are compared as presented; rows A and B through the frames next to them."""
    a, b, c = expected["A"]["frames"], expected["B"]["frames"], expected["C"]["frames"]
    e, f = expected["E"]["frames"], expected["F"]["frames"]                  # E as A; F presents f[3k + 1 .. 3k + 3], factors 0.3 and 0.7
    for k in CUTS:                                   # call k + 1 presents a[4k + 1 .. 4k + 4], b[3k + 1 .. 3k + 3], c[2k + 1 .. 2k + 2]
        assert hc.same(a[4 * k + 1], a[4 * k]) and hc.same(a[4 * k + 2], a[4 * k + 4]) and hc.same(a[4 * k + 3], a[4 * k + 4])
        assert hc.same(e[4 * k + 1], e[4 * k]) and hc.same(e[4 * k + 2], e[4 * k + 4]) and hc.same(e[4 * k + 3], e[4 * k + 4])
        assert hc.same(f[3 * k + 1], f[3 * k]) and hc.same(f[3 * k + 2], f[3 * k + 3])
        assert hc.same(b[3 * k + 2], b[3 * k + 1]) and hc.same(b[3 * k + 3], b[3 * k + 1])
        assert hc.same(c[2 * k + 1], c[2 * k + 2])
    for k in (1,):                                   # the one pair that is no cut
        assert not hc.same(a[4 * k + 1], a[4 * k]) and not hc.same(a[4 * k + 2], a[4 * k + 4])
        assert not hc.same(e[4 * k + 1], e[4 * k]) and not hc.same(e[4 * k + 2], e[4 * k + 4])
        assert not hc.same(f[3 * k + 1], f[3 * k]) and not hc.same(f[3 * k + 2], f[3 * k + 3])
        assert not hc.same(b[3 * k + 2], b[3 * k + 1]) and not hc.same(c[2 * k + 1], c[2 * k + 2])


@pytest.mark.parametrize("name", ROW_IDS)
def test_expected_frames_are_pairwise_distinct(expected, name):
    """A stale or swapped slot shows: no two presented frames hold the same bytes -- but for the frames a cut repeats, which by
    definition are the real frame next to them (test_a_cut_shows_source_frames) and no other."""
    e = expected[name]
    repeated = len(hc.the_factors(hc.ROW[name])) * e["cuts"]
    assert len({packed(f) for f in e["frames"]}) == e["presented"] - repeated


DROPPED = [("A", o) for o in ("motion", "refine-vectors", "interpolator", "protect-static", "cut-threshold", "sharpen", "input-format",
                              "output-format", "yuv")] + \
          [("B", o) for o in ("generation", "cut-threshold", "sharpen", "input-format", "output-format")] + \
          [("E", o) for o in ("motion", "refine-vectors", "interpolator", "bidirectional", "half-res-motion", "hole-reach", "cut-threshold",
                              "sharpen", "output-format")] + \
          [("F", o) for o in ("interpolator", "subpel-vectors", "half-res-motion", "cut-threshold")] + \
          [("G", o) for o in ("motion", "refine-vectors", "interpolator", "protect-static", "hole-reach", "input-format", "output-format")]


@pytest.mark.parametrize("name,option", DROPPED, ids=[f"{n}-{o}" for n, o in DROPPED])
def test_every_option_shows_on_this_stream(frames, expected, name, option):
    """Each option of the all-on rows, taken away alone, changes a presented frame or the cut count.  (Row A's --semantics and
    row B's --interpolator are not options to drop: the pyramid, the refinement and the compensated interpolator depend on
    neither semantics, by the header's definition, and extrapolation needs the compensated interpolator.  Row F's --motion full
    is lfg_host's default: there is nothing to take away.  Row G's --scale-filter: test_the_scale_filter_shows_where_the_loop_scales.)"""
    full, less = expected[name], hc.expected_cpu(frames, hc.without(hc.ROW[name], option))
    assert less["presented"] == full["presented"]
    changed = sum(not hc.same(x, y) for x, y in zip(full["frames"], less["frames"]))
    print(f"row {name} without {option}: {changed} of {full['presented']} frames change, cuts {full['cuts']} -> {less['cuts']}")
    assert changed > 0 or less["cuts"] != full["cuts"]
    if option not in ("cut-threshold", "generation"):        # the settings of a generated frame show on one: pair (1, 2) is no cut
        at = {"A": range(5, 8), "B": range(5, 7), "E": range(5, 8), "F": range(4, 6), "G": range(3, 4)}[name]
        assert any(not hc.same(full["frames"][i], less["frames"][i]) for i in at), "no generated frame of the moving pair changes"


def test_the_scale_filter_shows_where_the_loop_scales(oracle, frames):
    """Row G's --scale-filter lanczos3.  At output size = input size, where the CPU models can state the whole stream, Lanczos-3
    is the identity -- sinc vanishes at every whole offset but 0, so each sample is its centre tap alone -- and taking the option
    away changes no frame: stated here so that nobody looks for it.  Where the loop scales, it shows: the reference's scale is a
    Lanczos-3 of its own, with another window and edge rule, and at 2x the filter's frame leaves the oracle's by more than the
    1 LSB within which lfg_scale is held to the oracle; on the GPU
    test_gpu_host_schedules.py: test_the_scale_filter_shows_on_the_large_stream compares the two streams."""
    from tests import resample_model as rsm
    row = hc.ROW["G"]
    less = hc.expected_cpu(frames, hc.without(row, "scale-filter"))
    assert all(hc.same(x, y) for x, y in zip(hc.expected_cpu(frames, row)["frames"], less["frames"]))
    assert (hc.scaled_cpu(frames[1], row) == frames[1]).all()
    twice = rsm.resample(frames[1], 2 * W, 2 * H, rsm.LANCZOS3).astype(int) - oracle.scale(frames[1], 2 * W, 2 * H).astype(int)
    print(f"lanczos3 against the reference scale at 2x: {int((abs(twice) > 1).any(-1).sum())} of {4 * W * H} pixels beyond 1 LSB")
    assert (abs(twice) > 1).any()


def test_options_are_lfg_hosts(expected):
    assert hc.options(hc.ROW["A"]) == ["--semantics", "intended", "--interpolator", "compensated", "--motion", "pyramid", "--refine-vectors", "1",
                                       "--factors", "0.25,0.5,0.75", "--protect-static", "0", "--cut-threshold", "500", "--sharpen", "24",
                                       "--input-format", "nv12", "--output-format", "nv12", "--yuv-matrix", "601", "--yuv-range", "full",
                                       "--chroma", "replicate"]
    assert hc.options(hc.ROW["B"]) == ["--semantics", "intended", "--interpolator", "compensated", "--motion", "full", "--factors", "0.5,1.0",
                                       "--generation", "extrapolate", "--cut-threshold", "500", "--sharpen", "24", "--input-format", "nv12",
                                       "--output-format", "nv12"]
    assert hc.options(hc.ROW["C"]) == ["--semantics", "reference", "--interpolator", "shader", "--motion", "full", "--cut-threshold", "500",
                                       "--sharpen", "24"]
    assert hc.options(hc.ROW["D"]) == ["--semantics", "intended", "--interpolator", "compensated", "--motion", "full", "--output-format", "nv12"]
    assert hc.options(hc.ROW["E"]) == ["--semantics", "intended", "--interpolator", "compensated", "--motion", "pyramid", "--refine-vectors", "1",
                                       "--factors", "0.25,0.5,0.75", "--bidirectional", "1", "--half-res-motion", "1", "--hole-reach", "32",
                                       "--cut-threshold", "500", "--sharpen", "24", "--output-format", "nv12"]
    assert hc.options(hc.ROW["F"]) == ["--semantics", "intended", "--interpolator", "compensated", "--motion", "full", "--factors", "0.3,0.7",
                                       "--half-res-motion", "0", "--subpel-vectors", "1", "--cut-threshold", "500"]
    assert hc.options(hc.ROW["G"]) == ["--semantics", "intended", "--interpolator", "compensated", "--motion", "pyramid", "--refine-vectors", "1",
                                       "--protect-static", "0", "--hole-reach", "32", "--scale-filter", "lanczos3", "--input-format", "nv12",
                                       "--output-format", "nv12"]
    assert [s[0] for s in hc.SCHEDULES] == ["sync1", "lanes1", "lanes2", "lanes3", "sync3"]


def test_the_runner_starts_nothing_after_a_run_that_hung_or_died(monkeypatch, tmp_path):
    """gpu_kit.host_run with lfg_host stood in for: after a time-out, and after a death from a signal, the next call fails
    without starting anything; a run that merely fails (exit status 1) does not close the door."""
    import subprocess
    import sys
    from types import SimpleNamespace

    from tests import gpu_kit

    started = []

    def fake(outcome):
        def run(command, **kw):
            started.append(command)
            if outcome == "hang":
                raise subprocess.TimeoutExpired(command, kw["timeout"])
            return SimpleNamespace(returncode=outcome, stdout="", stderr="stood in for")
        return run

    monkeypatch.setattr(gpu_kit, "HOST", sys.executable)               # exists: nothing is built
    frame = [np.zeros((4, 4, 4), np.uint8)]
    for outcome in ("hang", -11):
        monkeypatch.setattr(gpu_kit, "_host_failed", None)
        monkeypatch.setattr(gpu_kit.subprocess, "run", fake(1))
        with pytest.raises(AssertionError):
            gpu_kit.host_run(tmp_path, frame, (4, 4))
        assert gpu_kit._host_failed is None
        monkeypatch.setattr(gpu_kit.subprocess, "run", fake(outcome))
        with pytest.raises(pytest.fail.Exception):
            gpu_kit.host_run(tmp_path, frame, (4, 4), timeout=7)
        assert gpu_kit._host_failed
        count = len(started)
        with pytest.raises(pytest.fail.Exception, match="not started again"):
            gpu_kit.host_run(tmp_path, frame, (4, 4))
        assert len(started) == count
