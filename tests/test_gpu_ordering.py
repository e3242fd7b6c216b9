"""The calls whose whole job is ordering -- lfg_lane_mark / _wait / _sync, lfg_sync across lanes, lfg_lanes shrinking, the ring's
upload / download / wait / fence / acquire, lfg_context_set_stream / _get_stream -- held to the happens-before model of
tests/order_cases.py on the GPU.  Bytes after an lfg_sync cannot show them: every schedule here puts a blocker of milliseconds
in front of the write its read must see, reads back through pinned memory and the wait under test alone, and runs a second time
as its control, without the ordering call -- which must then show the OTHER content.  A control that does not is a failed test:
the streams ran in turn and the schedule's pass means nothing.

All of it runs in one child process (tests/order_runner.py), started once, with eight hardware queues for its six streams; the
tests below read its records."""
import json
import os
import subprocess
import sys

import pytest

from tests import gpu_kit
from tests import order_cases as oc
from tests.host_cli import ROOT

pytestmark = pytest.mark.gpu

ROUNDS = 3
GPU_CONTROLS = [s for s in oc.SCHEDULES if s.control is not None and (s.control_expect or s.control_busy)]


@pytest.fixture(scope="module")
def records():
    """{(schedule, round, control): record} of the one run.  A run that times out or dies from a signal may have left the GPU in a
    state in which the next child does the same: none is started again in the session (gpu_kit.host_run's rule, and its flag)."""
    if gpu_kit._host_failed:
        pytest.fail(f"no child process is started again in this session: {gpu_kit._host_failed}", pytrace=False)
    command = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.order_runner"]
    try:
        p = subprocess.run(command, cwd=ROOT, env=dict(os.environ, GPU_MAX_HW_QUEUES="8"), capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        gpu_kit._host_failed = "tests.order_runner did not end within 240 s"
        pytest.fail(gpu_kit._host_failed, pytrace=False)
    if p.returncode < 0:
        gpu_kit._host_failed = f"tests.order_runner died from signal {-p.returncode}"
        pytest.fail(gpu_kit._host_failed + "\n" + p.stderr[-2000:], pytrace=False)
    assert p.returncode == 0, p.stderr[-4000:]
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            out[r["schedule"], r.get("round", 0), r.get("control", False)] = r
    c = out["calibration", 0, False]
    print(f"blocker: {c['blockers']} lfg_motion call(s), {c['blocker_ms']:.3f} ms on the device; longest enqueue {c['enqueue_ms']:.3f} ms; "
          f"ratio {c['ratio']:.0f}; three rounds took {out['destroyed', 0, False]['seconds']:.2f} s")
    return out


def test_the_blocker_outlasts_every_enqueue(records):
    """Device time of the blocker against the host time of the longest schedule's enqueue, both measured in the child: 50 times
    over when the blocker was sized, and never less than once over in any run that is judged below."""
    c = records["calibration", 0, False]
    assert c["ok"], f"{c['blockers']} blockers last {c['blocker_ms']:.3f} ms, the longest enqueue {c['enqueue_ms']:.3f} ms: a ratio of {c['ratio']:.1f}, not 50"
    for key, r in records.items():
        if "enqueue_ms" in r and key[0] != "calibration":
            print(key, f"enqueue {r['enqueue_ms']:.3f} ms, blocker {r['blocker_ms']:.3f} ms")
            assert r["enqueue_ms"] < r["blocker_ms"], key


@pytest.mark.parametrize("rnd", range(ROUNDS))
@pytest.mark.parametrize("s", oc.SCHEDULES, ids=lambda s: s.name)
def test_a_schedule_reads_what_the_rules_determine(records, s, rnd):
    r = records[s.name, rnd, False]
    assert r["reads"] == s.expect, (s.rule, r)
    assert r["busy"] == {str(k): v for k, v in s.busy.items()}, (s.rule, r)


@pytest.mark.parametrize("rnd", range(ROUNDS))
@pytest.mark.parametrize("s", GPU_CONTROLS, ids=lambda s: s.name)
def test_its_control_reads_the_other_content(records, s, rnd):
    """The same ops without the ordering call: the read must see the other write, or the schedule's pass meant nothing."""
    r = records[s.name, rnd, True]
    seen = {b: r["reads"][b] for b in s.control_expect}
    assert seen == s.control_expect and r["busy"] == {str(k): v for k, v in s.control_busy.items()}, \
        f"vacuous: the streams ran in turn ({s.name}, without its {s.rule} call: {r})"


@pytest.mark.parametrize("rnd", range(ROUNDS))
def test_an_adopted_stream(records, rnd):
    """lfg_context_set_stream / _get_stream beyond the schedules: the handles, lfg_interpolate_frames under route_cases.BASE on the
    adopted stream against RouteChain, NULL and handle 0, and the stream's owner after lfg_lanes(ctx, 1)."""
    checks = records["adopted", rnd, False]["checks"]
    assert len(checks) == 8 and all(checks.values()), checks


def test_the_adopted_stream_outlives_the_context(records):
    checks = records["destroyed", 0, False]["checks"]
    assert len(checks) == 3 and all(checks.values()), checks
