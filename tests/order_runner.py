"""`python -m tests.order_runner`: the schedules of tests/order_cases.py on the GPU, in a process of their own.

Started once per session by tests/test_gpu_ordering.py with GPU_MAX_HW_QUEUES=8.  Its one context is the first of the process; it
uses at most three lanes, one ring (of one slot) and two caller streams -- six streams on eight hardware queues, so that no two of
them share a queue and run in turn.  Every schedule runs ROUNDS times as written and ROUNDS times as its control (the same ops
without the ordering call under test); one JSON record per run goes to stdout, each with the host time the schedule took to
enqueue and the device time of its blocker.  Read-backs go through lfg_frame_download into pinned memory and the wait under test,
never through Context.download (an lfg_sync).

The blocker is lfg_motion on uncorrelated 1280 x 720 frames, repeated until its device time is at least RATIO times the longest
enqueue time (at most MAX_BLOCKERS calls): a racing op given to an idle stream then runs long before the blocker ends."""
import ctypes
import json
import sys
import time

import numpy as np

from linux_fg_amd import capi, synth
from tests import order_cases as oc
from tests import route_cases as rc
from tests.big_views import hip_runtime

W, H = 320, 180
ROUNDS, RATIO, MAX_BLOCKERS = 3, 50.0, 8
HIP_NOT_READY = 600                                  # hipErrorNotReady
HOST_WAITS = ("lane_sync", "sync", "ring_wait", "ring_acquire", "lanes", "read")


class Hip:
    """The caller's own HIP calls, on the runtime the library is bound to."""

    def __init__(self):
        self.rt = hip_runtime()
        p, pp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
        for name, args in {"hipStreamCreateWithFlags": [pp, ctypes.c_uint], "hipStreamDestroy": [p], "hipEventCreateWithFlags": [pp, ctypes.c_uint],
                           "hipEventDestroy": [p], "hipEventRecord": [p, p], "hipStreamWaitEvent": [p, p, ctypes.c_uint], "hipStreamQuery": [p],
                           "hipEventQuery": [p], "hipEventSynchronize": [p],
                           "hipEventElapsedTime": [ctypes.POINTER(ctypes.c_float), p, p]}.items():
            fn = getattr(self.rt, name)
            fn.restype, fn.argtypes = ctypes.c_int, args

    def ok(self, rc, what):
        assert rc == 0, f"{what}: HIP error {rc}"

    def stream(self):
        s = ctypes.c_void_p()
        self.ok(self.rt.hipStreamCreateWithFlags(ctypes.byref(s), 1), "hipStreamCreateWithFlags")      # hipStreamNonBlocking
        return s.value

    def event(self, timing=False):
        e = ctypes.c_void_p()
        self.ok(self.rt.hipEventCreateWithFlags(ctypes.byref(e), 0 if timing else 2), "hipEventCreateWithFlags")      # hipEventDisableTiming
        return e.value

    def record(self, event, stream):
        self.ok(self.rt.hipEventRecord(event, stream), "hipEventRecord")

    def stream_wait(self, stream, event):
        self.ok(self.rt.hipStreamWaitEvent(stream, event, 0), "hipStreamWaitEvent")

    def busy(self, stream):
        rc = self.rt.hipStreamQuery(stream)
        assert rc in (0, HIP_NOT_READY), f"hipStreamQuery: HIP error {rc}"
        return rc == HIP_NOT_READY

    def elapsed_ms(self, first, last):
        self.ok(self.rt.hipEventSynchronize(last), "hipEventSynchronize")
        assert self.rt.hipEventQuery(last) == 0
        ms = ctypes.c_float()
        self.ok(self.rt.hipEventElapsedTime(ctypes.byref(ms), first, last), "hipEventElapsedTime")
        return float(ms.value)


class Rig:
    """The context, its frames and pinned buffers, and the interpreter of order_cases' ops."""

    def __init__(self, ctx, hip):
        self.ctx, self.hip, self.blockers, self.warm = ctx, hip, 1, set()
        small = {name: synth.make_prev(W, H, seed=7300 + k) for k, name in enumerate(("old", "new", "A", "B"))}
        big = {"X": synth.make_prev(2 * W, 2 * H, seed=7310), "poison": np.full((2 * H, 2 * W, 4), 0x5A, np.uint8)}
        self.frames = {"F": ctx.create_frame(W, H), **{n: ctx.create_frame(2 * W, 2 * H) for n in ("U", "U2", "G")}}
        for name in ("old", "new"):                  # what lfg_scale gives alone on an idle context
            ctx.upload(self.frames["F"], small[name])
            ctx.scale(self.frames["F"], self.frames["U"])
            big[f"s({name})"] = ctx.download(self.frames["U"]).copy()
        self.content = {**{k: v.reshape(-1) for k, v in small.items()}, **{k: v.reshape(-1) for k, v in big.items()}}
        self.content["poison_small"] = self.content["poison"][:W * H * 4]
        self.n_big = 4 * W * H * 4
        self.host = {n: ctx.staging_create(self.n_big) for n in ("P", "P2", "PX")}
        self.host["Pf"] = ctx.staging_create(W * H * 4)
        self.ring = ctx.ring_create(1, self.n_big)
        self.host["slot"], self.slot = self.ring.acquire()
        a, b = synth.make_uncorrelated_pair(1280, 720, stream=3)
        self.pair = ctx.frame_from(a), ctx.frame_from(b)
        self.mv = [ctx.create_frame(1280, 720, capi.FORMAT_MV_S8X2) for _ in range(3)]
        self.streams = {"S": hip.stream(), "T": hip.stream()}
        self.events = {"E": hip.event()}
        self.timing = hip.event(True), hip.event(True)

    def handle(self, name):
        if not name.startswith("lane:"):
            return self.streams[name]
        at = self.ctx.lane_current()
        self.ctx.lane_select(int(name[5:]))
        h = self.ctx.get_stream()
        self.ctx.lane_select(at)
        return h

    def block(self):
        for _ in range(self.blockers):
            self.ctx.motion(*self.pair, self.mv[self.ctx.lane_current()], 8, 16.0)

    def prepare(self, lanes, init):
        """`lanes` lanes, each with its motion workspace made (the first call of a lane allocates), lane 0 selected, every
        output and every pinned buffer poisoned."""
        ctx = self.ctx
        ctx.lane_select(0)
        if ctx.lane_count() != lanes:
            ctx.lanes(lanes)
            self.warm = {j for j in self.warm if j < lanes}
        for j in set(range(lanes)) - self.warm:
            ctx.lane_select(j)
            ctx.motion(*self.pair, self.mv[j], 8, 16.0)
            self.warm.add(j)
        ctx.lane_select(0)
        for name, f in self.frames.items():
            ctx.upload(f, self.content[init.get(name, "poison_small" if name == "F" else "poison")])
        ctx.sync()
        for a in self.host.values():
            a[:] = 0x5A

    def drain(self):
        ctx = self.ctx
        ctx.sync()
        self.ring.wait(self.slot)
        for j in range(ctx.lane_count()):
            ctx.lane_select(j)
            ctx.set_stream(None)
        ctx.lane_select(0)
        ctx.sync()

    def name_of(self, got):
        for name, c in self.content.items():
            if c.size == got.size and (c == got).all():
                return "poison" if name == "poison_small" else name
        return "mixed"

    def run(self, ops):
        """(what each ("read", buf) saw, by content name; what each ("query", s) answered; host ms from the blocker's first
        call to the first call that waits)."""
        ctx, frames, host = self.ctx, self.frames, self.host
        reads, busy, begun, enqueue = {}, {}, None, None
        for k, (kind, *a) in enumerate(ops):
            if kind in HOST_WAITS and begun is not None and enqueue is None:
                enqueue = (time.perf_counter() - begun) * 1e3
            if kind == "select":
                ctx.lane_select(a[0])
            elif kind == "lanes":
                ctx.lanes(a[0])
                self.warm = {j for j in self.warm if j < a[0]}
            elif kind == "mark":
                ctx.lane_mark()
            elif kind == "wait":
                ctx.lane_wait(a[0])
            elif kind == "lane_sync":
                ctx.lane_sync()
            elif kind == "sync":
                ctx.sync()
            elif kind == "adopt":
                ctx.set_stream(self.streams[a[0]] if a[0] else None)
            elif kind == "block" and a:
                ctx.motion(*self.pair, self.mv[ctx.lane_current()], 8, 16.0)
            elif kind == "block":
                begun = begun or time.perf_counter()
                self.block()
            elif kind == "run":
                what, src, dst = a
                if what == "scale":
                    ctx.scale(frames[src], frames[dst])
                elif what == "copy":
                    ctx.copy(frames[src], frames[dst])
                elif what == "upload":
                    ctx.upload_async(frames[dst], host[src])
                else:
                    assert what == "download", what
                    ctx.download_async(frames[src], host[dst][:frames[src].height * frames[src].pitch])
            elif kind == "ring_upload":
                self.ring.upload(self.slot, frames[a[0]])
            elif kind == "ring_download":
                self.ring.download(self.slot, frames[a[0]])
            elif kind == "ring_wait":
                self.ring.wait(self.slot)
            elif kind == "ring_fence":
                self.ring.fence_slot(self.slot)
            elif kind == "ring_acquire":
                assert self.ring.acquire()[1] == self.slot
            elif kind == "fill":
                c = self.content[a[1]]
                host[a[0]][:c.size] = c
            elif kind == "read":
                n = W * H * 4 if a[0] == "Pf" else self.n_big
                reads[a[0]] = self.name_of(host[a[0]][:n].copy())
            elif kind == "record":
                self.hip.record(self.events[a[0]], self.handle(a[1]))
            elif kind == "stream_wait":
                self.hip.stream_wait(self.handle(a[0]), self.events[a[1]])
            elif kind == "query":
                busy[k] = self.hip.busy(self.handle(a[0]))
            else:
                assert kind == "nop", kind
        return reads, busy, enqueue

    def blocker_ms(self):
        """Device time of the blocker alone on lane 0, between two events."""
        self.prepare(2, {})
        stream = self.ctx.get_stream()
        self.hip.record(self.timing[0], stream)
        self.block()
        self.hip.record(self.timing[1], stream)
        ms = self.hip.elapsed_ms(*self.timing)
        self.drain()
        return ms

    def schedule(self, s, control):
        self.prepare(s.lanes, s.init)
        reads, busy, enqueue = self.run(oc.control_ops(s) if control else s.ops)
        self.drain()
        return {"reads": reads, "busy": {str(k): v for k, v in busy.items()}, "enqueue_ms": enqueue}


def emit(**record):
    print(json.dumps(record), flush=True)


def has_gpu_control(s):
    return s.control is not None and bool(s.control_expect or s.control_busy)


def adopted(rig, chain, want, scene, out, pinned):
    """What the schedules cannot say about lfg_context_set_stream / lfg_context_get_stream: the handles, an lfg_interpolate_frames
    call with the lane's temporaries on the adopted stream, NULL and 0, and whose the stream is after the lane has gone."""
    from tests.test_gpu_routes import restore, select
    ctx, hip, (S, T), checks = rig.ctx, rig.hip, (rig.streams["S"], rig.streams["T"]), {}
    rig.prepare(2, {})
    own0 = ctx.get_stream()
    ctx.lane_select(1)
    own1 = ctx.get_stream()
    ctx.set_stream(0)                                # handle 0 on a lane that has adopted nothing: still its own
    checks["handle 0 adopts nothing"] = ctx.get_stream() == own1 and own1 != 0
    ctx.lane_select(0)
    ctx.set_stream(S)
    checks["get_stream returns the adopted stream"] = ctx.get_stream() == S and S not in (own0, own1)
    ctx.lane_select(1)
    checks["the other lane's stream is unchanged"] = ctx.get_stream() == own1
    ctx.set_stream(T)
    ctx.lane_select(0)
    select(ctx, chain, rc.route(rc.BASE))
    ctx.interpolate_frames(*scene, out, 0.5)
    ctx.download_async(out, pinned)
    ctx.lane_sync()
    checks["lfg_interpolate_frames on the adopted stream equals the chain"] = bool((pinned == want.reshape(-1)).all())
    ctx.set_stream(0)                                # handle 0 restores
    checks["handle 0 restores the lane's own stream"] = ctx.get_stream() == own0
    ctx.set_stream(S)
    ctx.set_stream(None)
    checks["NULL returns the lane's own handle"] = ctx.get_stream() == own0
    rig.block()
    checks["the next call runs on the lane's own stream"] = hip.busy(own0) and not hip.busy(S)
    ctx.sync()
    ctx.set_stream(S)
    restore(ctx)                                     # lfg_lanes(ctx, 1): lane 1, which had adopted T, goes
    rig.warm &= {0}
    hip.record(rig.events["E"], T)
    hip.ok(rig.hip.rt.hipEventSynchronize(rig.events["E"]), "an event on T after its lane has gone")
    checks["after lfg_lanes(ctx, 1) the adopted stream is still the caller's"] = not hip.busy(T) and ctx.get_stream() == S
    rig.drain()
    return checks


def main():
    chain = rc.scene_chain()
    want = chain.frames(rc.route(rc.BASE), [0.5])[0]
    hip = Hip()
    ctx = capi.Context(0)
    rig = Rig(ctx, hip)
    scene = ctx.frame_from(chain.prev), ctx.frame_from(chain.curr)
    out = ctx.create_frame(want.shape[1], want.shape[0])
    pinned = ctx.staging_create(want.size)
    runs = [(s, control) for s in oc.SCHEDULES for control in (False, True) if not control or has_gpu_control(s)]
    # the blocker: as many calls as it takes to outlast the longest enqueue RATIO times over, both measured here
    for rig.blockers in range(1, MAX_BLOCKERS + 1):
        enqueue = max(min(rig.schedule(s, control)["enqueue_ms"] for _ in range(2)) for s, control in runs)      # (the better of two: a hiccup of the host is what RATIO is the margin for)
        device = rig.blocker_ms()
        if device >= RATIO * enqueue:
            break
    emit(schedule="calibration", blockers=rig.blockers, blocker_ms=device, enqueue_ms=enqueue, ratio=device / enqueue,
         ok=device >= RATIO * enqueue)
    began = time.perf_counter()
    for rnd in range(ROUNDS):
        for s, control in runs:
            emit(schedule=s.name, round=rnd, control=control, blockers=rig.blockers, blocker_ms=device, **rig.schedule(s, control))
        emit(schedule="adopted", round=rnd, control=False, checks=adopted(rig, chain, want, scene, out, pinned))
    seconds = time.perf_counter() - began
    # after lfg_context_destroy the adopted stream is still the caller's
    ctx.set_stream(rig.streams["S"])
    rig.ring.destroy()
    ctx.close()
    S, T = rig.streams["S"], rig.streams["T"]
    checks = {"after lfg_context_destroy the adopted stream answers hipSuccess": hip.rt.hipStreamQuery(S) == 0,
              "hipStreamDestroy of it succeeds": hip.rt.hipStreamDestroy(S) == 0, "and of the other": hip.rt.hipStreamDestroy(T) == 0}
    for e in list(rig.events.values()) + list(rig.timing):
        hip.ok(hip.rt.hipEventDestroy(e), "hipEventDestroy")
    emit(schedule="destroyed", round=0, control=False, checks=checks, seconds=seconds)


if __name__ == "__main__":
    sys.exit(main())
