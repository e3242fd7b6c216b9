"""lfg_motion_pyramid on the GPU against the CPU model (tests/pyramid_model.py), byte for byte; its argument checks; the
estimator switch of lfg_interpolate_frames[_multi]; lanes; the host's --motion / --semantics options; and the tie case of
test_pyramid_model.py."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import pyramid_model as pm
from tests.gpu_kit import ctx, host_run, pitched, three_lanes

pytestmark = pytest.mark.gpu

PARAMS = [(1, 32, 1), (2, 16, 2), (3, 12, 3), (4, 7, 1), (2, 8, 4)]
SIZES = [(1, 1), (7, 5), (33, 17), (64, 64), (257, 131)]


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "translated":
        prev = synth.make_prev(w, h, synth.BASE_SEED + seed)
        shift = tuple(int(v) for v in rng.integers(-60, 61, 2))
        return prev, synth.translate(prev, shift, synth.BASE_SEED + seed)
    if kind == "uncorrelated":
        return synth.make_uncorrelated_pair(w, h, seed)
    if kind == "identical":
        prev = synth.make_prev(w, h, synth.BASE_SEED + seed)
        return prev, prev.copy()
    flat = np.full((h, w, 4), rng.integers(0, 256, 4, dtype=np.uint8), np.uint8)
    return flat, flat.copy()


def run_pyramid(ctx, prev, curr, params):
    h, w = prev.shape[:2]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    ctx.motion_pyramid(p, c, m, *params)
    out = ctx.download(m)
    for f in (p, c, m):
        ctx.destroy_frame(f)
    return out


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("kind", ["translated", "uncorrelated", "identical", "flat"])
def test_every_pixel_equals_the_model(ctx, params, kind):
    for i, (w, h) in enumerate(SIZES):
        prev, curr = content(kind, w, h, 11 * i + 3)
        got = run_pyramid(ctx, prev, curr, params)
        want = pm.motion_pyramid(prev, curr, *params)
        bad = np.argwhere((got != want).any(-1))
        assert bad.size == 0, f"{w}x{h} {params} {kind}: {len(bad)} pixels differ, first {bad[:3].tolist()}"


@pytest.mark.parametrize("axis", [0, 1])
def test_tie_between_equal_length_vectors(ctx, axis):
    """test_pyramid_model.py's tie (tests/cases.py): v and -v match exactly; the smaller vy or, vy equal, the smaller vx wins.
    With more levels the tie is decided on reduced images first: those run against the model as well."""
    prev, curr, params, want = cases.pyramid_tie(axis)
    got = run_pyramid(ctx, prev, curr, params)
    assert (got == pm.motion_pyramid(prev, curr, *params)).all()
    inner = got[12:-12, 12:-12].reshape(-1, 2)
    assert (inner == np.array(want, np.int8)).all(), np.unique(inner, axis=0)
    for other in PARAMS:
        assert (run_pyramid(ctx, prev, curr, other) == pm.motion_pyramid(prev, curr, *other)).all(), other


@pytest.mark.parametrize("params", [(2, 16, 2), (4, 7, 1)])
def test_padded_pitch_640x360(ctx, params):
    w, h, pad = 640, 360, 12
    prev, curr = content("translated", w, h, 7)
    bp, p = pitched(ctx, prev, pad)
    bc, c = pitched(ctx, curr, pad)
    bm, m = pitched(ctx, np.zeros((h, w, 2), np.int8), pad, capi.FORMAT_MV_S8X2)
    ctx.motion_pyramid(p, c, m, *params)
    raw = ctx.download(bm)
    assert (raw[:, w:].view(np.uint8) == 0x5A).all()                 # the padding is not written
    assert (raw[:, :w] == pm.motion_pyramid(prev, curr, *params)).all()
    for f in (bp, bc, bm):
        ctx.destroy_frame(f)


def test_1080p_rois_and_4k(ctx):
    for (w, h), n in (((1920, 1080), 12), ((3840, 2160), 16)):
        prev, curr = content("translated", w, h, 21)
        got = run_pyramid(ctx, prev, curr, (2, 16, 2))
        rng = np.random.default_rng(w)
        rois = [(0, 0, 64, 64), (w - 64, h - 64, 64, 64)] + [(int(rng.integers(0, w - 64)), int(rng.integers(0, h - 64)), 64, 64) for _ in range(n - 2)]
        for x, y, rw, rh in rois:
            want = pm.motion_pyramid(prev, curr, 2, 16, 2, roi=(x, y, rw, rh))
            assert (got[y:y + rh, x:x + rw] == want).all(), (w, h, x, y)


@pytest.mark.parametrize("shift,need", [((40, -24), 1.0), ((37, -29), 0.99)])
def test_4k_pan(ctx, shift, need):
    w, h = 3840, 2160
    prev = synth.make_prev(w, h)
    curr = synth.translate(prev, shift)
    got = run_pyramid(ctx, prev, curr, (2, 16, 2))
    sx, sy = shift
    inner = got[max(0, sy) + 64:h + min(0, sy) - 64, max(0, sx) + 64:w + min(0, sx) - 64].reshape(-1, 2)
    frac = float((inner == np.array([-sx, -sy], np.int8)).all(-1).mean())
    print(f"4K shift {shift}: {100 * frac:.3f} % of interior pixels exact")
    assert frac >= need


def test_invalid_arguments_launch_nothing(ctx):
    lib = ctx.lib
    w, h = 40, 24
    prev, curr = content("translated", w, h, 1)
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    pattern = np.full((h, w, 2), 0x5A, np.int8)
    ctx.upload(m, pattern)
    for params in ((0, 16, 2), (5, 4, 1), (2, 0, 2), (2, 33, 2), (2, 16, 0), (2, 16, 5), (2, 31, 2)):
        rc = lib.lfg_motion_pyramid(ctx.h, ctypes.byref(p), ctypes.byref(c), ctypes.byref(m), *params)
        assert rc == -4, params                                  # LFG_ERR_UNSUPPORTED
        assert lib.lfg_last_error(ctx.h).decode()
    small = ctx.create_frame(w - 1, h, capi.FORMAT_MV_S8X2)
    rgba_mv = ctx.create_frame(w, h)
    cases = [(p, c, rgba_mv), (m, c, m), (p, c, small)]
    for a, b, o in cases:
        rc = lib.lfg_motion_pyramid(ctx.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(o), 2, 16, 2)
        assert rc == -1                                          # LFG_ERR_INVALID
        assert lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_set_motion_estimator(ctx.h, 2) == -1 and lib.lfg_last_error(ctx.h).decode()
    ctx.sync()
    assert (ctx.download(m) == pattern).all()
    for f in (p, c, m, small, rgba_mv):
        ctx.destroy_frame(f)


def _interp_cases():
    w, h = 640, 360
    yield "640x360", synth.make_pair(w, h, shift=(23, -41))
    W, H = 3840, 2160
    prev = synth.make_prev(W, H)
    yield "4k", (prev, synth.translate(prev, (-52, 30)))


def test_interpolation_with_the_pyramid_estimator(ctx, oracle):
    factors = [0.25, 0.5, 0.75]
    for name, (prev, curr) in _interp_cases():
        h, w = prev.shape[:2]
        x, y, rw, rh = (0, 0, w, h) if name == "640x360" else (1700, 900, 96, 64)
        mv = np.zeros((h, w, 2), np.float32)
        mv[y:y + rh, x:x + rw] = pm.motion_pyramid(prev, curr, 2, 16, 2, roi=(x, y, rw, rh))
        p, c = ctx.frame_from(prev), ctx.frame_from(curr)
        outs = [ctx.create_frame(w, h) for _ in factors]
        try:
            ctx.set_semantics(capi.SEMANTICS_INTENDED)
            ctx.set_motion_estimator(capi.ESTIMATOR_PYRAMID)
            for fused in (False, True):
                ctx.set_fused_motion_interpolate(fused)
                ctx.interpolate_frames(p, c, outs[0], 0.5)
                single = ctx.download(outs[0])
                ctx.interpolate_frames_multi(p, c, outs, factors)
                multi = [ctx.download(o) for o in outs]
                for t, got in [(0.5, single)] + list(zip(factors, multi)):
                    want = oracle.interpolate(prev, curr, mv, t, roi=(x, y, x + rw, y + rh), semantics=oracle.INTENDED)
                    assert (got[y:y + rh, x:x + rw] == want[y:y + rh, x:x + rw]).all(), (name, fused, t)
            # back to the full search: lfg_motion + lfg_interpolate again
            ctx.set_fused_motion_interpolate(False)
            ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
            ctx.interpolate_frames(p, c, outs[0], 0.5)
            got = ctx.download(outs[0])
            m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
            ctx.motion(p, c, m)
            ctx.interpolate(p, c, m, outs[1], 0.5)
            assert (got == ctx.download(outs[1])).all()
            ctx.destroy_frame(m)
        finally:
            ctx.set_motion_estimator(capi.ESTIMATOR_FULL_SEARCH)
            ctx.set_semantics(capi.SEMANTICS_REFERENCE)
            ctx.set_fused_motion_interpolate(False)
            for f in [p, c] + outs:
                ctx.destroy_frame(f)


def test_three_lanes_equal_one_lane(ctx):
    sizes = [(200, 120), (96, 64), (200, 120), (130, 90), (96, 64), (130, 90)]
    pairs = [content("translated" if i % 2 else "uncorrelated", w, h, 40 + i) for i, (w, h) in enumerate(sizes)]
    alone = [run_pyramid(ctx, a, b, (2, 16, 2)) for a, b in pairs]

    def enqueue(i, a, b):
        h, w = a.shape[:2]
        p, c = ctx.frame_from(a), ctx.frame_from(b)
        m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
        ctx.motion_pyramid(p, c, m, 2, 16, 2)
        return p, c, m

    three_lanes(ctx, pairs, enqueue, alone)


def test_host_pyramid_stream_matches_capi(tmp_path):
    w, h, n = 1920, 1080, 3
    frames = [synth.make_prev(w, h)]
    for k in range(1, n):
        frames.append(synth.translate(frames[-1], (20, 0), synth.BASE_SEED + k))
    _, got = host_run(tmp_path, frames, (w, h), "--semantics", "intended", "--motion", "pyramid")
    assert len(got) == 2 * n - 1
    with capi.Context(0) as c:
        c.set_semantics(capi.SEMANTICS_INTENDED)
        ins = [c.frame_from(f) for f in frames]
        ups = [c.create_frame(w, h) for _ in frames]
        for i, u in zip(ins, ups):
            c.scale(i, u)
        m = c.create_frame(w, h, capi.FORMAT_MV_S8X2)
        o = c.create_frame(w, h)
        want = [c.download(ups[0])]
        for k in range(1, n):
            c.motion_pyramid(ups[k - 1], ups[k], m, 2, 16, 2)
            c.interpolate(ups[k - 1], ups[k], m, o, 0.5)
            want += [c.download(o), c.download(ups[k])]
    for k, (g, e) in enumerate(zip(got, want)):
        assert (g == e).all(), k
