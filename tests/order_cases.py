"""The ordering calls of include/linuxfg_hip.h as a happens-before model, and the schedules that hold the library to it on the GPU
(tests/order_runner.py runs them, tests/test_gpu_ordering.py judges them, tests/test_order_model.py holds them to the model).
Written from the header and INTEGRATION.md, not from lfg_capi.cpp.  Nothing here needs a GPU.

The rules, each an edge of the graph that `graph` builds and each removable by name:
  R1   a stream is in order with itself
  R2   lfg_lane_wait(i): the selected lane's later work waits for lane i's LAST mark -- not for what lane i was given after it, and
       for nothing before lane i's first mark
  R3   lfg_lane_sync: the host waits for the selected lane alone
  R4   lfg_sync: the host waits for every lane, adopted streams included
  R5   a ring upload is ordered after the selected lane's earlier work
  R6   ... and before the selected lane's later work
  R7   a ring download is ordered after the selected lane's earlier work; later work does not wait for it
  R8   lfg_ring_fence_slot: later work on the selected lane waits for the slot's last transfer
  R9   lfg_ring_acquire, lfg_ring_wait: the host waits for the slot's last transfer
  R10  lfg_context_set_stream: the selected lane's calls run on the adopted stream (NULL: on its own again)
  R11  lfg_lanes(ctx, fewer): the host waits for the lanes that go

An op is a tuple, made in host program order:
  ("select", j)  ("lanes", n)  ("mark",)  ("wait", i)  ("lane_sync",)  ("sync",)  ("adopt", "S" | None)  ("nop",)
  ("block",)                       the blocker on the selected lane: milliseconds of lfg_motion on frames of its own
  ("block", 1)                     one call of it: a millisecond that keeps a read-back from being there at once, on a lane that
                                   has to end long before another lane's blocker does
  ("run", kind, src, dst)          scale | copy | upload (pinned -> frame) | download (frame -> pinned) on the selected lane
  ("ring_upload", dst)  ("ring_download", src)  ("ring_wait",)  ("ring_fence",)  ("ring_acquire",)      the one slot: buffer "slot"
  ("fill", buf, content)  ("read", buf)        the host writes / reads pinned memory
  ("record", "E", stream)  ("stream_wait", stream, "E")      the caller's own HIP calls; a stream is "S", "T" or "lane:j"
  ("query", stream)                hipStreamQuery; the model ignores it
"""
from collections import namedtuple

RULES = tuple(f"R{k}" for k in range(1, 12))
INIT = -1                                            # the write that put a buffer's first content there, before the schedule


def graph(ops, rules=RULES):
    """(preds, reads, writes, node_of): the happens-before graph of `ops` under `rules`.  A node is ("host", k) -- op k returning
    to the caller -- or ("dev", k), what op k put on a stream; node_of[k] is the one that touches op k's buffers."""
    preds, reads, writes, node_of = {INIT: set()}, {}, {}, {}
    own = {j: f"own{j}" for j in range(4)}           # lane -> the stream the library made for it (idle lanes order nothing)
    stream, tail, mark, event = dict(own), {}, {}, {}
    sel, slot_last, host, made = 0, None, INIT, 1

    def node(key, *before, r=(), w=()):
        preds[key] = {b for b in before if b is not None}
        reads[key], writes[key] = tuple(r), tuple(w)
        return key

    def on(k, s, *before, r=(), w=()):               # a device node of op k on stream s
        n = node(("dev", k), ("host", k), tail.get(s) if "R1" in rules else None, *before, r=r, w=w)
        tail[s] = n
        return n

    def named(s):
        return stream[int(s[5:])] if s.startswith("lane:") else s

    for k, (kind, *a) in enumerate(ops):
        h = node(("host", k), host)
        node_of[k] = host = h
        cur = stream[sel]
        if kind == "select":
            sel = a[0]
        elif kind == "lanes":
            for j in [j for j in stream if j >= a[0]]:
                if "R11" in rules:
                    preds[h] |= {tail.get(stream[j]), tail.get(own[j])} - {None}
                del stream[j], own[j]
                mark.pop(j, None)
            for j in range(len(stream), a[0]):
                own[j] = stream[j] = f"own{j}.{made}"
                made += 1
            sel = sel if sel < a[0] else 0
        elif kind == "mark":
            mark[sel] = on(k, cur)
        elif kind == "wait":
            if a[0] != sel and a[0] in mark:
                on(k, cur, mark[a[0]] if "R2" in rules else None)
        elif kind == "lane_sync":
            preds[h] |= {tail.get(cur)} - {None} if "R3" in rules else set()
        elif kind == "sync":
            preds[h] |= {tail.get(s) for s in stream.values()} - {None} if "R4" in rules else set()
        elif kind == "adopt":
            if "R10" in rules:
                stream[sel] = a[0] or own[sel]
        elif kind == "block":
            node_of[k] = on(k, cur)
        elif kind == "run":
            node_of[k] = on(k, cur, r=[a[1]], w=[a[2]])
        elif kind in ("ring_upload", "ring_download"):
            up = kind == "ring_upload"
            rule = "R5" if up else "R7"
            t = node(("dev", k), h, tail.get(cur) if rule in rules else None, r=["slot" if up else a[0]], w=[a[0] if up else "slot"])
            node_of[k] = slot_last = t
            if up and "R6" in rules:
                tail[cur] = node(("join", k), t, tail.get(cur))
        elif kind == "ring_fence":
            on(k, cur, slot_last if "R8" in rules else None)
        elif kind in ("ring_wait", "ring_acquire"):
            preds[h] |= {slot_last} - {None} if "R9" in rules else set()
        elif kind == "fill":
            writes[h] = (a[0],)
        elif kind == "read":
            reads[h] = (a[0],)
        elif kind == "record":
            event[a[0]] = on(k, named(a[1]))
        elif kind == "stream_wait":
            on(k, named(a[0]), event[a[1]])
        else:
            assert kind in ("nop", "query"), kind
    return preds, reads, writes, node_of


def before(preds, n):
    """Every node that happens before n."""
    seen, todo = set(), list(preds[n])
    while todo:
        m = todo.pop()
        if m not in seen:
            seen.add(m)
            todo += preds[m]
    return seen


def sees(ops, k, buf, rules=RULES):
    """(the ops whose write of `buf` op k's read can see, whether a write races it): INIT stands for the first content.  The read
    is determined where that is one op and no race."""
    preds, reads, writes, node_of = graph(ops, rules)
    r = node_of[k]
    assert buf in reads[r], (ops[k], buf)
    op_of = {n: j for j, n in node_of.items()}
    earlier = before(preds, r)
    writers = [n for n in writes if buf in writes[n] and n != r] + [INIT]
    visible = [w for w in writers if w in earlier]
    latest = [w for w in visible if not any(w in before(preds, v) for v in visible if v != w)]
    race = any(w not in earlier and r not in before(preds, w) for w in writers)
    return sorted(op_of.get(w, INIT) for w in latest), race


def ordered_after(ops, k, j, rules=RULES):
    """Does op k (the host's return from it, or what it enqueued) happen after what op j enqueued?"""
    preds, _, _, node_of = graph(ops, rules)
    return node_of[j] in before(preds, node_of[k])


def all_reads(ops):
    preds, reads, _, node_of = graph(ops)
    return [(k, b) for k, n in node_of.items() for b in reads.get(n, ())]


# ---- the schedules

# rule: the rule the schedule is named for (None: a schedule that shows what a rule does NOT order -- it has `not_after`);
# read: (op, buffer), the single read; sees: the op whose write it must see; control: {op: its replacement} -- the same ops without
# the ordering call under test (None: there is none to run, `why` says why); not_after: (op, op) the first must not be ordered
# after the second; lanes: the lanes the context has when the schedule starts; init: first contents other than poison;
# expect / control_expect: what the host reads at the end, by buffer; busy / control_busy: what the ("query", s) ops must answer.
Schedule = namedtuple("Schedule", "name rule ops read sees control lanes init expect control_expect not_after busy control_busy why")


def schedule(name, rule, ops, read, sees, control=None, lanes=2, init=None, expect=None, control_expect=None, not_after=None,
             busy=None, control_busy=None, why=""):
    return Schedule(name, rule, tuple(ops), read, sees, control, lanes, dict({"F": "old"}, **(init or {})), expect or {},
                    control_expect or {}, not_after, busy or {}, control_busy or {}, why)


def control_ops(s):
    return tuple(s.control.get(k, op) for k, op in enumerate(s.ops))


NOP = ("nop",)
_READ_G = [("run", "copy", "U", "G"), ("run", "download", "G", "P"), ("lane_sync",), ("read", "P")]


def _mark_wait(waiter, adopt=()):
    ops = list(adopt) + [("select", 0), ("block",), ("run", "scale", "F", "U"), ("mark",), ("select", waiter), ("wait", 0)] + _READ_G
    at = len(adopt)
    return ops, (at + 6, "U"), at + 2, {at + 5: NOP}


def _ring_upload(lane, adopt=()):
    """blocker; scale(F -> U); [nop] ring_upload(slot -> F) [nop]; scale(F -> U2); both read back.  The nops are where the controls
    select the other lane, so that the upload (R5) or the work after it (R6) is no longer the selected lane's."""
    ops = list(adopt) + [("fill", "slot", "new"), ("select", lane), ("block",), ("run", "scale", "F", "U"), NOP, ("ring_upload", "F"), NOP,
                         ("run", "scale", "F", "U2"), ("run", "download", "U", "P"), ("run", "download", "U2", "P2"), ("lane_sync",),
                         ("read", "P"), ("read", "P2")]
    return ops, len(adopt)


def _schedules():
    out = []
    S0 = [("select", 0), ("adopt", "S")]
    ops, read, seen, control = _mark_wait(1)
    out.append(schedule("mark_wait", "R2", ops, read, seen, control, expect={"P": "s(old)"}, control_expect={"P": "poison"}))
    out.append(schedule(
        "wait_is_for_the_mark_not_the_end", "R2",
        [("select", 0), ("run", "scale", "F", "U"), ("mark",), ("block",), ("select", 1), ("wait", 0)] + _READ_G + [("query", "lane:0")],
        (6, "U"), 1, {5: NOP}, expect={"P": "s(old)"}, not_after=(9, 3), busy={10: True},
        why="the upscale in front of the blocker is done long before lane 1 reads: with the wait left out the bytes are the same; "
            "what is observed is that the wait ends before lane 0 does"))
    out.append(schedule(
        "second_mark_supersedes", "R2",
        [("select", 0), ("mark",), ("block",), ("run", "scale", "F", "U"), ("mark",), ("select", 1), ("wait", 0)] + _READ_G,
        (7, "U"), 3, {4: NOP}, expect={"P": "s(old)"}, control_expect={"P": "poison"}))
    out.append(schedule(
        "wait_before_any_mark_and_on_itself", None,
        [("lanes", 1), ("lanes", 2), ("select", 1), ("block", 1), ("lane_sync",), ("block",), ("select", 0), ("wait", 1), ("wait", 0),
         ("run", "scale", "F", "U"), ("run", "download", "U", "P"), ("lane_sync",), ("read", "P"), ("query", "lane:1")],
        (12, "P"), 10, None, expect={"P": "s(old)"}, not_after=(12, 5), busy={13: True},
        why="nothing is ordered: there is no call to leave out.  Lane 1 is new, so it has never marked; its first, short call makes its workspace"))
    ops, read, seen, control = _mark_wait(2)
    out.append(schedule("mark_wait_three_lanes", "R2", ops, read, seen, control, lanes=3, expect={"P": "s(old)"}, control_expect={"P": "poison"}))
    out.append(schedule(
        "lane_sync", "R3",
        [("select", 0), ("block",), ("select", 1), ("block", 1), ("run", "scale", "F", "U"), ("run", "download", "U", "P"), ("lane_sync",),
         ("read", "P"), ("query", "lane:0")],
        (7, "P"), 5, {6: NOP}, expect={"P": "s(old)"}, control_expect={"P": "poison"}, not_after=(7, 1), busy={8: True}, control_busy={8: True}))
    out.append(schedule(
        "sync_every_lane", "R4",
        [("select", 2), ("adopt", "S"), ("block",), ("select", 0), ("block", 1), ("run", "scale", "F", "U"), ("run", "download", "U", "P"),
         ("select", 1), ("sync",), ("read", "P"), ("query", "lane:0"), ("query", "lane:1"), ("query", "S")],
        (9, "P"), 6, {8: NOP}, lanes=3, expect={"P": "s(old)"}, control_expect={"P": "poison"},
        busy={10: False, 11: False, 12: False}, control_busy={10: True, 11: False, 12: True}))
    out.append(schedule(
        "shrink_waits_for_the_lanes_that_go", "R11",
        [("select", 2), ("block",), ("run", "scale", "F", "U"), ("lanes", 1), ("run", "download", "U", "P"), ("lane_sync",), ("read", "P")],
        (4, "U"), 2, None, lanes=3, expect={"P": "s(old)"}, why="without the wait the lane's workspace would be freed under its kernels"))
    for lane in (0, 1):
        ops, at = _ring_upload(lane)
        both = {"P": "s(old)", "P2": "s(new)"}
        out.append(schedule(f"ring_upload_after_earlier_work_lane{lane}", "R5", ops, (at + 3, "F"), INIT,
                            {at + 4: ("select", 1 - lane), at + 6: ("select", lane)}, expect=both, control_expect={"P": "s(new)"}))
        out.append(schedule(f"ring_upload_before_later_work_lane{lane}", "R6", ops, (at + 7, "F"), at + 5,
                            {at + 6: ("select", 1 - lane)}, expect=both, control_expect={"P2": "s(old)"}))
    down = [("select", 0), ("block",), ("run", "scale", "F", "U"), NOP, ("ring_download", "U"), NOP, ("ring_wait",), ("read", "slot")]
    out.append(schedule("ring_download_after_its_producers", "R7", down, (4, "U"), 2, {3: ("select", 1), 5: ("select", 0)},
                        expect={"slot": "s(old)"}, control_expect={"slot": "poison"}))
    out.append(schedule("ring_wait", "R9", down, (7, "slot"), 4, {6: NOP}, expect={"slot": "s(old)"}, control_expect={"slot": "poison"}))
    out.append(schedule(
        "fence_holds_an_overwrite_back", "R8",
        [("fill", "PX", "X"), ("select", 0), ("run", "scale", "F", "U"), ("block",), ("ring_download", "U"), ("select", 1), ("ring_fence",),
         ("run", "upload", "PX", "U"), ("ring_wait",), ("read", "slot")],
        (4, "U"), 2, {6: NOP}, expect={"slot": "s(old)"}, control_expect={"slot": "X"}))
    out.append(schedule(
        "acquire_blocks_on_a_busy_slot", "R9",
        [("ring_acquire",), ("fill", "slot", "A"), ("select", 0), ("block",), ("ring_upload", "F"), ("ring_acquire",), ("fill", "slot", "B"),
         ("run", "download", "F", "Pf"), ("sync",), ("read", "Pf")],
        (4, "slot"), 1, {5: NOP}, expect={"Pf": "A"}, control_expect={"Pf": "B"}))
    out.append(schedule(
        "adopted_stream_waits_for_the_callers_event", "R10",
        S0 + [("select", 1), ("block",), ("run", "scale", "F", "U"), ("record", "E", "lane:1"), ("stream_wait", "S", "E"), ("select", 0)] + _READ_G,
        (8, "U"), 4, {6: NOP}, expect={"P": "s(old)"}, control_expect={"P": "poison"}))
    out.append(schedule(
        "callers_stream_waits_for_the_adopted_one", "R10",
        S0 + [("select", 1), ("adopt", "T"), ("select", 0), ("block",), ("run", "scale", "F", "U"), ("record", "E", "S"), ("stream_wait", "T", "E"),
              ("select", 1)] + _READ_G,
        (10, "U"), 6, {8: NOP}, expect={"P": "s(old)"}, control_expect={"P": "poison"}))
    ops, read, seen, control = _mark_wait(1, adopt=S0)
    out.append(schedule("mark_wait_on_an_adopted_stream", "R2", ops, read, seen, control, expect={"P": "s(old)"}, control_expect={"P": "poison"}))
    ops, at = _ring_upload(0, adopt=S0)
    out.append(schedule("ring_upload_on_an_adopted_stream", "R5", ops, (at + 3, "F"), INIT, {at + 4: ("select", 1), at + 6: ("select", 0)},
                        expect={"P": "s(old)", "P2": "s(new)"}, control_expect={"P": "s(new)"}))
    return out


SCHEDULES = _schedules()
BY_NAME = {s.name: s for s in SCHEDULES}
assert len(BY_NAME) == len(SCHEDULES)


def frames_in_flight(lanes, n_frames=7):
    """tests/test_gpu_parity.py::test_lanes_keep_frames_in_flight_apart as ops: frame k on lane k % lanes waits for the other lane's
    mark, upscales into ups[k], marks, and measures motion between ups[k - 1] and ups[k].  Returns (ops, the reads of ups[k - 1]
    as (op, buffer, the op whose write it must see))."""
    ops, reads, wrote = [("lanes", lanes)], [], {}
    for k in range(n_frames):
        ops += [("select", k % lanes), ("wait", (k - 1) % lanes), ("run", "scale", f"in{k}", f"up{k}"), ("mark",)]
        wrote[k] = len(ops) - 2
        if k:
            ops.append(("run", "motion", f"up{k - 1}", f"mv{k}"))
            reads.append((len(ops) - 1, f"up{k - 1}", wrote[k - 1]))
    return ops, reads
