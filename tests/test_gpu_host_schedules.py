"""lfg_host's loop (host/scaler.cpp, frame_manager.cpp, main.cpp) held to the chain with every stage on, under every schedule:
the option rows and the stream of tests/host_stream_cases.py, every presented byte and the report's counts.

Anchor.  Rows A to G at 96 x 64, output = input, 6 frames, one lane with --sync-present: every presented byte equals the CPU
models' (host_stream_cases.expected_cpu), and so does the same stream made through capi.Context one call at a time
(expected_capi), which is the reference of the larger tier.

Schedules.  Rows A to G under all five schedules at 640 x 360 -> 1280 x 720 with 12 frames.  Twelve frames is a condition, not a
tuning knob.  Scaler::Initialize gives the read-back ring (1 + lanes) * (factors + 1) + 2 slots, and --sharpen and
--output-format nv12 keep one buffer per slot (m_sharpened, m_nv12Out); the upload ring has 2 + lanes slots and every lane one
NV12 staging buffer (m_nv12In):

    lanes  factors  read-back slots  presented = 1 + 11 * (factors + 1)
      3       3          18               45      (rows A, E)
      3       2          14               34      (rows B, F)
      3       1          10               23      (rows C, D, G)
      1       3          10               45

The upload ring's 5 slots (3 lanes) take 12 uploads and each lane's staging buffer 4 or more.  So every slot, every per-slot
buffer and every lane's staging buffer is used again at least twice in every run -- each test asserts presented > 2 * slots for
its lanes and factors -- where every earlier host test with one of these options stopped before the first reuse.  The stream
cuts at its first pair, at two consecutive pairs in the middle and at its last pair, so the cut count is read on each of its
three paths (one call late with one lane, at presentation with several lanes or --sync-present, at Flush for the last pair)
next to a cut that the neighbouring call must not count again.

Sizes and time.  720p rather than the suite's usual tiny host frames so that kernels and transfers overlap at all.  A logic
error -- a wrong index, order or count -- fails at any size, every time.  A missing fence fails only when the timing allows it:
a pass here does not prove that every fence is there, and the tests do not repeat runs to look for one."""
import os

import pytest

from tests import host_stream_cases as hc
from tests.gpu_kit import ctx, host_run

pytestmark = pytest.mark.gpu

ROW_IDS = [r["name"] for r in hc.ROWS]
BIG_IN, BIG_OUT, BIG_N = (640, 360), (1280, 720), 12
FIELDS = ("presented", "interpolated", "cuts", "in_flight", "input_format", "output_format", "sharpen")


def check(info, got, want, row, n, in_flight, what):
    """The report's fields and every presented frame, byte for byte."""
    fields = dict(hc.report_fields(row, n), cuts=want["cuts"], in_flight=in_flight)
    assert {k: info.get(k) for k in FIELDS} == fields, what
    assert (want["presented"], want["interpolated"]) == (fields["presented"], fields["interpolated"]), what
    assert len(got) == want["presented"], what
    bad = [i for i, (g, e) in enumerate(zip(got, want["frames"])) if not hc.same(g, e)]
    assert not bad, f"{what}: presented frames {bad} of {len(got)} differ (generated: {[want['flags'][i] for i in bad]})"


# ---- the anchor

@pytest.fixture(scope="module")
def small(oracle):
    frames = hc.stream(*hc.SMALL)
    return frames, {r["name"]: hc.expected_cpu(frames, r) for r in hc.ROWS}


@pytest.mark.parametrize("name", ROW_IDS)
def test_anchor_equals_the_cpu_models(small, tmp_path, name):
    frames, expected = small
    row, (w, h, n) = hc.ROW[name], hc.SMALL
    _, options, _, in_flight = hc.SCHEDULES[0]
    info, got = host_run(tmp_path / name, hc.inputs(frames, row), (w, h), *hc.options(row), *options, timeout=60)
    assert info["pipelined"] is False
    check(info, got, expected[name], row, n, in_flight, f"row {name}")


@pytest.mark.parametrize("name", ROW_IDS)
def test_capi_chain_equals_the_cpu_models(ctx, small, name):
    """What the schedule tests compare with is the models' stream."""
    frames, expected = small
    row, (w, h, _) = hc.ROW[name], hc.SMALL
    got, want = hc.expected_capi(ctx, frames, row, (w, h)), expected[name]
    assert {k: got[k] for k in ("flags", "cut_at", "cuts", "presented", "interpolated")} == \
           {k: want[k] for k in ("flags", "cut_at", "cuts", "presented", "interpolated")}
    bad = [i for i, (g, e) in enumerate(zip(got["frames"], want["frames"])) if not hc.same(g, e)]
    assert not bad, f"row {name}: frames {bad} differ"


# ---- the schedules

@pytest.fixture(scope="module")
def big(ctx):
    """The 12-frame stream, what lfg_host is fed of it per row, and the chain's stream per row, each computed once."""
    frames = hc.stream(*BIG_IN, BIG_N)
    fed = {r["name"]: hc.inputs(frames, r) for r in hc.ROWS}
    want = {r["name"]: hc.expected_capi(ctx, frames, r, BIG_OUT) for r in hc.ROWS}
    return fed, want


@pytest.mark.parametrize("name", ROW_IDS)
def test_the_large_stream_cuts_where_it_is_made_to(big, name):
    """Upscaled to 720p the stream still cuts at its four pairs (the rows with detection on), and the chain's frames tell a stale slot: all
    distinct but for the frames a cut repeats."""
    want = big[1][name]
    row = hc.ROW[name]
    assert want["cut_at"] == (list(hc.cut_pairs(BIG_N)) if row["threshold"] >= 0 else [])
    parts = {b"".join(p.tobytes() for p in (f if isinstance(f, tuple) else (f,))) for f in want["frames"]}
    assert len(parts) == want["presented"] - len(hc.the_factors(row)) * want["cuts"]


def test_the_scale_filter_shows_on_the_large_stream(ctx, big):
    """Row G's --scale-filter lanczos3 is the identity at the anchor's output size = input size (test_host_stream_cases.py:
    test_the_scale_filter_shows_where_the_loop_scales); here, where the loop scales by 2, the chain without it presents other
    bytes in every frame, so a loop that dropped the option would fail row G's schedules."""
    row = hc.ROW["G"]
    frames = hc.stream(*BIG_IN, BIG_N)[:3]
    less = hc.expected_capi(ctx, frames, hc.without(row, "scale-filter"), BIG_OUT)
    with_filter = big[1]["G"]["frames"][:less["presented"]]
    assert less["presented"] == 5 and not any(hc.same(x, y) for x, y in zip(with_filter, less["frames"]))


@pytest.mark.parametrize("schedule", hc.SCHEDULES, ids=[s[0] for s in hc.SCHEDULES])
@pytest.mark.parametrize("name", ROW_IDS)
def test_schedule_presents_the_chain(big, tmp_path, name, schedule):
    fed, want = big
    row = hc.ROW[name]
    sid, options, lanes, in_flight = schedule
    info, got = host_run(tmp_path / f"{name}-{sid}", fed[name], BIG_OUT, *hc.options(row), *options, timeout=60)
    assert info["pipelined"] is ("--sync-present" not in options)
    assert info["presented"] > 2 * hc.readback_slots(lanes, row), "the run is too short to use every slot twice again"
    check(info, got, want[name], row, BIG_N, in_flight, f"{name}-{sid}")


# ---- the interpolated flag of each presented frame, under both presentation orders

@pytest.mark.parametrize("name,per_call", [("B", ["real", "interp", "interp"]), ("A", ["interp", "interp", "interp", "real"])])
def test_dump_names_follow_the_presentation_order(small, tmp_path, name, per_call):
    frames, expected = small
    row, (w, h, n) = hc.ROW[name], hc.SMALL
    dump = tmp_path / "dump"
    dump.mkdir()
    info, got = host_run(tmp_path / "run", hc.inputs(frames, row), (w, h), *hc.options(row), "--dump-dir", str(dump), timeout=60)
    names = sorted(os.listdir(dump))
    kinds = [f.split("_")[2] for f in names]
    assert [f.split("_")[1] for f in names] == [f"{i:04d}" for i in range(info["presented"])]
    assert kinds == ["real"] + per_call * (n - 1)
    assert kinds == ["interp" if flag else "real" for flag in expected[name]["flags"]]
    assert all(f.endswith(f"_{w}x{h}.nv12") for f in names)
    check(info, got, expected[name], row, n, 2, f"row {name} with --dump-dir")           # (the default schedule: two lanes)
