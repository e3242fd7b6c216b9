"""The schedules of tests/order_cases.py held to its happens-before model, without a GPU: every schedule's read is determined
under the header's rules, the rule a schedule is named for is what determines it, every control is a race, and the schedule of
test_lanes_keep_frames_in_flight_apart is determined too."""
import pytest

from tests import order_cases as oc

IDS = [s.name for s in oc.SCHEDULES]


def carried(ops, read, seen, rule):
    """Is the read determined with every rule, and no longer (a race, or another write) with `rule` taken out?"""
    if oc.sees(ops, *read) != ([seen], False):
        return False
    return oc.sees(ops, *read, rules=[r for r in oc.RULES if r != rule]) != ([seen], False)


@pytest.mark.parametrize("s", oc.SCHEDULES, ids=IDS)
def test_every_read_of_a_schedule_is_determined(s):
    assert oc.sees(s.ops, *s.read) == ([s.sees], False)
    for k, buf in oc.all_reads(s.ops):                       # the read-back behind it as well
        writers, race = oc.sees(s.ops, k, buf)
        assert len(writers) == 1 and not race, (s.ops[k], buf, writers, race)
    assert s.expect and all(s.ops[k][0] == "query" for k in list(s.busy) + list(s.control_busy))
    assert {op[1] for op in s.ops if op[0] == "read"} == set(s.expect)


@pytest.mark.parametrize("s", oc.SCHEDULES, ids=IDS)
def test_the_rule_a_schedule_is_named_for_carries_it(s):
    if s.rule is None:                                       # a schedule of what is NOT ordered: nothing carries it ...
        assert s.not_after and s.control is None
        return
    assert carried(s.ops, s.read, s.sees, s.rule)


@pytest.mark.parametrize("s", oc.SCHEDULES, ids=IDS)
def test_what_a_rule_does_not_order(s):
    if s.not_after:
        k, j = s.not_after
        assert not oc.ordered_after(s.ops, k, j)
        assert s.ops[j] == ("block",)                        # the blocker, not its one-call form


@pytest.mark.parametrize("s", [s for s in oc.SCHEDULES if s.control is not None], ids=lambda s: s.name)
def test_every_control_is_a_race(s):
    ops = oc.control_ops(s)
    assert ops != s.ops and len(ops) == len(s.ops)
    writers, race = oc.sees(ops, *s.read)
    assert race, (s.name, writers)
    assert bool(s.control_expect or s.control_busy) == (not s.why), "a control runs on the GPU, or `why` says why not"
    assert all(s.expect[b] != c for b, c in s.control_expect.items())


def test_schedules_without_a_control_say_why():
    for s in oc.SCHEDULES:
        assert (s.control is None) <= bool(s.why), s.name
    assert [s.name for s in oc.SCHEDULES if s.control is None] == ["wait_before_any_mark_and_on_itself", "shrink_waits_for_the_lanes_that_go"]


def test_every_rule_has_a_schedule():
    assert {s.rule for s in oc.SCHEDULES} - {None} == set(oc.RULES) - {"R1"}


def test_a_schedule_its_rule_does_not_carry_is_noticed():
    """The mark in front of the upscale it should cover: the read is a race with R2 and without.  And the upscale on the waiting
    lane itself: determined with R2 and without.  Neither counts as carried."""
    s = oc.BY_NAME["mark_wait"]
    ops = list(s.ops)
    ops[2], ops[3] = ops[3], ops[2]
    assert not carried(ops, (s.read[0], "U"), 3, "R2")
    ops = [("select", 1) if op == ("select", 0) else op for op in s.ops]
    assert oc.sees(ops, *s.read) == ([s.sees], False) and not carried(ops, s.read, s.sees, "R2")


def test_removing_a_rule_from_the_model_fails_some_schedule():
    for rule in oc.RULES[1:]:
        rules = [r for r in oc.RULES if r != rule]
        assert any(oc.sees(s.ops, *s.read, rules=rules) != ([s.sees], False) for s in oc.SCHEDULES), rule


@pytest.mark.parametrize("lanes", [1, 2, 3])
def test_frames_in_flight_of_the_parity_suite_are_determined(lanes):
    """tests/test_gpu_parity.py::test_lanes_keep_frames_in_flight_apart: every motion call's read of the previous frame's upscale
    sees that upscale -- by R2 on two and three lanes, by R1 alone on one."""
    ops, reads = oc.frames_in_flight(lanes)
    assert len(reads) == 6
    for k, buf, wrote in reads:
        assert oc.sees(ops, k, buf) == ([wrote], False)
        without = oc.sees(ops, k, buf, rules=[r for r in oc.RULES if r != "R2"])
        assert (without == ([wrote], False)) == (lanes == 1)
