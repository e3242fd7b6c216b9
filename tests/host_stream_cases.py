"""The streams that hold lfg_host's loop (host/scaler.cpp: Scaler::ProcessFrame, QueueReadback, PresentPending, ReadCut) to the
chain, and what the loop must present of them: shared by tests/test_host_stream_cases.py (CPU: the cases can fail) and
tests/test_gpu_host_schedules.py (GPU: the loop under every schedule).

``stream(w, h, n)`` is the input, ``ROWS`` the seven option sets, ``SCHEDULES`` the five ways the loop can be scheduled,
``expected_cpu(frames, row)`` the presented stream from the CPU models alone (output size = input size, where the upscale is the
identity) and ``expected_capi(ctx, frames, row, out_size)`` the same stream through capi.Context, one call at a time on one
lane, at any output size.

The stream.  Every shift is even, in x and in y: NV12 carries one chroma pair per 2 x 2 pixels, so only an even shift of the
source is a shift of the converted frame, and only then do the vectors of a row with NV12 input match as they do on RGBA.  The
frames are windows into a larger canvas of synth noise (no exposed border to fill), panned by a shift that changes from frame to frame;
a textured square crosses them with a motion of its own; an overlay -- three one-pixel strokes and a block of noise aligned to
the chroma quads -- is drawn into every frame after the motion, at the same place with the same bytes.  A cut is a new canvas
seed.  What tests/pair_model.py reports of it (test_host_stream_cases.py asserts it, for every row, at 96 x 64 with 6 frames):
the four cut pairs match on 164 pixels per thousand or fewer (41 without NV12 input, whose chroma averaging brings unrelated
noise closer together), every other pair on 676 or more, against a threshold of 500: ROOM on both sides."""
from __future__ import annotations

import numpy as np

from linux_fg_amd import capi, synth
from tests import cases
from tests import pair_model as pair
from tests import resample_model as rsm
from tests import route_cases as rc
from tests import sharpen_model as sm
from tests import yuv_model as ym
from tests.test_gpu_cut import THRESHOLD

MATCH_SAD = 48                                      # what lfg_host gives lfg_set_interpolator
SMALL = (96, 64, 6)                                 # the stream of the CPU tests and of the anchor
ROOM = rc.ROOM                                      # pixels per thousand that every pair keeps between itself and the threshold

# ---- the stream

PANS = ((4, -2), (2, 2), (6, -4), (-2, 4), (4, 2))  # the window's step from frame k - 1 to frame k is PANS[k % 5]
SQUARE_STEP = (6, 2)                                # the square's, in frame coordinates, whatever the pan


def cut_pairs(n: int):
    """The pairs (k, k + 1), by k, across which the scene changes: the first, two consecutive ones in the middle, the last."""
    assert n >= 6, n
    m = (n - 1) // 2
    return (0, m, m + 1, n - 2)


def overlay(w: int, h: int):
    """(on, bytes): where the overlay is and what it holds."""
    on = np.zeros((h, w), bool)
    px = np.zeros((h, w, 4), np.uint8)
    on[6, 8:w // 2] = True
    on[10:h // 2, w - 10] = True
    on[h - 7, w // 3:2 * w // 3] = True
    px[on] = (255, 255, 255, 255)
    on[h - 20:h - 12, 8:20] = True                  # even origin, even size: whole chroma quads
    px[h - 20:h - 12, 8:20] = np.random.default_rng(3).integers(0, 256, (8, 12, 4), dtype=np.uint8)
    return on, px


def stream(w: int, h: int, n: int):
    """n pairwise-distinct RGBA frames of w x h (both even), with cuts at cut_pairs(n)."""
    assert w % 2 == 0 and h % 2 == 0 and w >= 64 and h >= 48, (w, h)
    cuts = cut_pairs(n)
    margin = 8 * n
    side = min(w, h) // 4 & ~1
    on, px = overlay(w, h)
    frames, scene = [], 0
    for k in range(n):
        if k == 0 or k - 1 in cuts:                 # a new scene: another canvas, window and square back at their origins
            scene += 1
            canvas = synth.noise_bytes(w + 2 * margin, h + 2 * margin, synth.BASE_SEED + 16 * scene)
            texture = cases.textured(side, side, 77 + scene)
            ox = oy = margin
            sx, sy = 16, 12
        else:
            ox, oy = ox + PANS[k % len(PANS)][0], oy + PANS[k % len(PANS)][1]
            sx, sy = sx + SQUARE_STEP[0], sy + SQUARE_STEP[1]
        f = canvas[oy:oy + h, ox:ox + w].copy()
        assert f.shape == (h, w, 4) and sx + side <= w and sy + side <= h, (k, ox, oy, sx, sy)
        f[sy:sy + side, sx:sx + side] = texture
        f[on] = px[on]
        frames.append(f)
    return frames


# ---- the rows: option sets of lfg_host.  A row is a dict; options(row) is its command line.

def _row(name, setting, factors=None, generation="interpolate", protect=-1, threshold=-1, sharpen=0, nv12_in=False, nv12_out=False,
         yuv=(ym.BT709, ym.LIMITED, ym.LEFT), bidirectional=-1, half_res=-1, hole_reach=-1, subpel=-1, scale_filter=None):
    """setting: (estimator, refinement radius, interpolator, semantics) as in tests/cases.py.  factors None: the single entry
    point at lfg_host's default of 0.5.  scale_filter: a name of tests/resample_model.py, None for lfg_scale."""
    return dict(name=name, setting=setting, factors=factors, generation=generation, protect=protect, threshold=threshold, sharpen=sharpen,
                nv12_in=nv12_in, nv12_out=nv12_out, yuv=yuv, bidirectional=bidirectional, half_res=half_res, hole_reach=hole_reach,
                subpel=subpel, scale_filter=scale_filter)


ROWS = [
    _row("A", ("pyramid", 1, "compensated", 1), factors=(0.25, 0.5, 0.75), protect=0, threshold=THRESHOLD, sharpen=24, nv12_in=True,
         nv12_out=True, yuv=(ym.BT601, ym.FULL, ym.REPLICATE)),
    _row("B", ("full", -1, "compensated", 1), factors=(0.5, 1.0), generation="extrapolate", threshold=THRESHOLD, sharpen=24, nv12_in=True,
         nv12_out=True),
    _row("C", ("full", -1, "shader", 0), threshold=THRESHOLD, sharpen=24),
    _row("D", ("full", -1, "compensated", 1), nv12_out=True),
    _row("E", ("pyramid", 1, "compensated", 1), factors=(0.25, 0.5, 0.75), bidirectional=1, half_res=1, hole_reach=32, threshold=THRESHOLD,
         sharpen=24, nv12_out=True),
    _row("F", ("full", -1, "compensated", 1), factors=(0.3, 0.7), subpel=1, half_res=0, threshold=THRESHOLD),
    # (with the refinement: on this stream of pure noise the pyramid alone matches the moving pair on 502 pixels per thousand,
    # which leaves no ROOM above the threshold that test_host_stream_cases.py measures every row against)
    _row("G", ("pyramid", 1, "compensated", 1), protect=0, hole_reach=32, scale_filter="lanczos3", nv12_in=True, nv12_out=True),
]
ROW = {r["name"]: r for r in ROWS}

SCHEDULES = [                                       # (id, options, lanes the loop runs with, what the report says of --in-flight)
    ("sync1", ("--in-flight", "1", "--sync-present"), 1, 1),
    ("lanes1", ("--in-flight", "1"), 1, 1),
    ("lanes2", ("--in-flight", "2"), 2, 2),
    ("lanes3", ("--in-flight", "3"), 3, 3),
    ("sync3", ("--in-flight", "3", "--sync-present"), 1, 3),     # falls back to one lane with a warning; the same stream
]


def the_factors(row):
    return tuple(row["factors"]) if row["factors"] else (0.5,)


def options(row):
    """The row as lfg_host's options (the sizes, the files and the schedule are the caller's)."""
    estimator, radius, interpolator, semantics = row["setting"]
    m, r, s = row["yuv"]
    out = ["--semantics", "intended" if semantics else "reference", "--interpolator", interpolator, "--motion", estimator]
    if radius >= 0:
        out += ["--refine-vectors", str(radius)]
    if row["factors"]:
        out += ["--factors", ",".join(repr(float(t)) for t in row["factors"])]
    if row["generation"] != "interpolate":
        out += ["--generation", row["generation"]]
    if row["protect"] >= 0:
        out += ["--protect-static", str(row["protect"])]
    for option, key in (("--bidirectional", "bidirectional"), ("--half-res-motion", "half_res"), ("--hole-reach", "hole_reach"),
                        ("--subpel-vectors", "subpel")):
        if row[key] >= 0:
            out += [option, str(row[key])]
    if row["threshold"] >= 0:
        out += ["--cut-threshold", str(row["threshold"])]
    if row["sharpen"]:
        out += ["--sharpen", str(row["sharpen"])]
    if row["scale_filter"]:
        out += ["--scale-filter", row["scale_filter"]]
    if row["nv12_in"]:
        out += ["--input-format", "nv12"]
    if row["nv12_out"]:
        out += ["--output-format", "nv12"]
    if row["yuv"] != (ym.BT709, ym.LIMITED, ym.LEFT):
        out += ["--yuv-matrix", "601" if m == ym.BT601 else "709", "--yuv-range", "full" if r == ym.FULL else "limited",
                "--chroma", "replicate" if s == ym.REPLICATE else "left"]
    return out


def without(row, option):
    """The row with one of its options back at lfg_host's default."""
    estimator, radius, interpolator, semantics = row["setting"]
    changed = {"motion": dict(setting=("full", radius, interpolator, semantics)),
               "refine-vectors": dict(setting=(estimator, -1, interpolator, semantics)),
               "interpolator": dict(setting=(estimator, radius, "shader", semantics)),
               "generation": dict(generation="interpolate"),
               "protect-static": dict(protect=-1), "cut-threshold": dict(threshold=-1), "sharpen": dict(sharpen=0),
               "bidirectional": dict(bidirectional=-1), "half-res-motion": dict(half_res=-1), "hole-reach": dict(hole_reach=-1),
               "subpel-vectors": dict(subpel=-1), "scale-filter": dict(scale_filter=None),
               "input-format": dict(nv12_in=False), "output-format": dict(nv12_out=False),
               "yuv": dict(yuv=(ym.BT709, ym.LIMITED, ym.LEFT))}[option]
    out = dict(row, **changed)
    assert out != row, f"row {row['name']} does not set {option}"
    return out


def inputs(frames, row):
    """What lfg_host is fed: the RGBA frames themselves, or with NV12 input their conversion by the model, as (y, uv)."""
    return [ym.rgba_to_nv12(f, *row["yuv"]) for f in frames] if row["nv12_in"] else list(frames)


def report_fields(row, n):
    """What the report says whatever the schedule ("sharpen" is left out of the report when it is off: None here)."""
    f = len(the_factors(row))
    return dict(presented=1 + (n - 1) * (f + 1), interpolated=(n - 1) * f, input_format="nv12" if row["nv12_in"] else "rgba",
                output_format="nv12" if row["nv12_out"] else "rgba", sharpen=row["sharpen"] or None)


def readback_slots(lanes, row):
    """Scaler::Initialize: the calls in flight, the one being presented, and a margin."""
    return (1 + lanes) * (len(the_factors(row)) + 1) + 2


def in_order(real, generated, row):
    """One call's frames as ProcessFrame queues them: ((frame, interpolated), ...)."""
    g = [(f, True) for f in generated]
    return [(real, False)] + g if row["generation"] == "extrapolate" else g + [(real, False)]


def same(a, b) -> bool:
    """Two presented frames, each an RGBA array or (y, uv), hold the same bytes."""
    if isinstance(a, tuple) != isinstance(b, tuple):
        return False
    return all(x.shape == y.shape and bool((x == y).all()) for x, y in (zip(a, b) if isinstance(a, tuple) else [(a, b)]))


# ---- the presented stream from the CPU models

_chains = {}


def chain_of(prev, curr):
    key = (prev.tobytes(), curr.tobytes())
    if key not in _chains:
        _chains[key] = rc.RouteChain(prev, curr)
    return _chains[key]


def route_of(row):
    """The row as a route of tests/route_cases.py: its threshold is a number, and the pair's record decides."""
    return rc.route(row["setting"], match_sad=MATCH_SAD, cut=row["threshold"] if row["threshold"] >= 0 else "off", generation=row["generation"],
                    protect=row["protect"], bidirectional=row["bidirectional"], half_res=row["half_res"], reach=row["hole_reach"],
                    subpel=row["subpel"])


def generated_cpu(prev, curr, row):
    """(the pair's generated frames, one per factor; its record, or None with detection off; whether it is a cut)."""
    chain, route = chain_of(prev, curr), route_of(row)
    detecting = row["threshold"] >= 0
    return chain.frames(route, the_factors(row)), (chain.stats(route) if detecting else None), detecting and chain.is_cut(route)


def scaled_cpu(frame, row):
    """The upscale at output size = input size: lfg_scale is the identity there; a filter of lfg_resample need not be."""
    if not row["scale_filter"]:
        return frame
    filt = {name: f for f, name in rsm.NAMES.items()}[row["scale_filter"]]
    return rsm.resample(frame, frame.shape[1], frame.shape[0], filt)


def presented_cpu(frame, row):
    """The sink: sharpened, then converted."""
    if row["sharpen"]:
        frame = sm.sharpen(frame, row["sharpen"])
    return ym.rgba_to_nv12(frame, *row["yuv"]) if row["nv12_out"] else frame


def expected_cpu(frames, row):
    """dict(frames, flags, cut_at, cuts, permille, presented, interpolated): what lfg_host presents of `frames` under `row` at the
    input size, each frame an RGBA array or (y, uv); flags[i] says whether frame i is a generated one, cut_at lists the cut
    pairs, permille each pair's matched pixels per thousand (None with detection off)."""
    real = [ym.nv12_to_rgba(*f, *row["yuv"]) for f in inputs(frames, row)] if row["nv12_in"] else list(frames)
    real = [scaled_cpu(f, row) for f in real]
    shown, cut_at, permille = [(real[0], False)], [], []
    for k in range(1, len(real)):
        generated, stats, is_cut = generated_cpu(real[k - 1], real[k], row)
        shown += in_order(real[k], generated, row)
        permille.append(None if stats is None else pair.permille(stats))
        if is_cut:
            cut_at.append(k - 1)
    flags = [flag for _, flag in shown]
    return dict(frames=[presented_cpu(f, row) for f, _ in shown], flags=flags, cut_at=cut_at, cuts=len(cut_at), permille=permille,
                presented=len(shown), interpolated=sum(flags))


# ---- the same stream through the C-ABI, one call at a time

def expected_capi(ctx, frames, row, out_size):
    """expected_cpu's dict (without permille) from capi.Context at out_size = (width, height): nv12_to_rgba, scale, the setters,
    (or resample), interpolate_frames or _multi, sharpen, rgba_to_nv12, last_pair_stats; one lane, a sync after every call.  Each of those calls
    is held to its model by its own test file: what this stands for is the chain, not the loop."""
    from tests.gpu_kit import DEFAULT, apply
    (h, w), (ow, oh) = frames[0].shape[:2], out_size
    factors = the_factors(row)
    made = []

    def new(*args):
        made.append(ctx.create_frame(*args))
        return made[-1]

    def sink(frame):
        if row["sharpen"]:
            ctx.sharpen(frame, sharp, row["sharpen"])
            frame = sharp
        if not row["nv12_out"]:
            return ctx.download(frame)                    # (download waits)
        ctx.rgba_to_nv12(frame, planes_out, *row["yuv"])
        ctx.sync()
        y, uv = ctx.download_nv12(nv12_out)
        return y.copy(), uv.copy()

    try:
        source, sharp = new(w, h), new(ow, oh)
        ups = [new(ow, oh), new(ow, oh)]
        outs = [new(ow, oh) for _ in factors]
        nv12_out, planes_out = ctx.create_nv12(ow, oh) if row["nv12_out"] else (None, None)
        if nv12_out is not None:
            made.append(nv12_out)
        apply(ctx, row["setting"], match_sad=MATCH_SAD, threshold=row["threshold"])
        ctx.set_static_protection(row["protect"])
        ctx.set_generation(capi.GENERATION_EXTRAPOLATE if row["generation"] == "extrapolate" else capi.GENERATION_INTERPOLATE)
        ctx.set_bidirectional(row["bidirectional"])
        ctx.set_half_resolution_motion(row["half_res"])
        ctx.set_hole_reach(row["hole_reach"])
        ctx.set_subpixel_vectors(row["subpel"])
        filt = {name: f for f, name in rsm.NAMES.items()}[row["scale_filter"]] if row["scale_filter"] else None
        shown, flags, cut_at = [], [], []
        for k, fed in enumerate(inputs(frames, row)):
            prev, curr = ups[(k + 1) % 2], ups[k % 2]
            if row["nv12_in"]:
                staged, planes = ctx.nv12_from(*fed)
                ctx.nv12_to_rgba(planes, source, *row["yuv"])
                ctx.sync()
                ctx.destroy_frame(staged)
            else:
                ctx.upload(source, fed)
            if filt is None:
                ctx.scale(source, curr)
            else:
                ctx.resample(source, curr, filt)
            ctx.sync()
            generated = []
            if k > 0:
                if row["factors"]:
                    ctx.interpolate_frames_multi(prev, curr, outs, factors)
                else:
                    ctx.interpolate_frames(prev, curr, outs[0], factors[0])
                ctx.sync()
                if row["threshold"] >= 0 and ctx.last_pair_stats()[1]:
                    cut_at.append(k - 1)
                generated = outs
            for frame, flag in in_order(curr, generated, row):
                shown.append(sink(frame))
                flags.append(flag)
        return dict(frames=shown, flags=flags, cut_at=cut_at, cuts=len(cut_at), presented=len(shown), interpolated=sum(flags))
    finally:
        ctx.sync()
        ctx.set_generation(capi.GENERATION_INTERPOLATE)
        for off in (ctx.set_static_protection, ctx.set_bidirectional, ctx.set_half_resolution_motion, ctx.set_hole_reach,
                    ctx.set_subpixel_vectors):
            off(-1)
        apply(ctx, DEFAULT)
        for f in made:
            ctx.destroy_frame(f)
