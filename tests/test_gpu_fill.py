"""The fill plane on the GPU (linux-fg_amd/csrc/hole_fill.hip), byte for byte against tests/fill_model.py: lfg_hole_fill_plane
on crafted key images, the compensated, masked and bidirectional calls under lfg_set_hole_reach, lfg_interpolate_frames_multi
on two lanes, and lfg_host --hole-reach."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import fill_cases as fc, fill_model as fm, mc_model as mc, overlay_model as ov, pyramid_model as pm
from tests.gpu_kit import DEFAULT, apply, ctx, first_bad, gpu_vectors, host_run, pitched

pytestmark = pytest.mark.gpu

MV = capi.FORMAT_MV_S8X2
# Partial waves and partial bands (fc.BAND = 64 rows, the column pass's band), a size that is whole in both, degenerate axes, and
# one in which reach 255 fits inside with more than one 256-pixel segment per row and five bands per column.
SIZES = [(130, 70), (67, 131), (64, 64), (1, 200), (200, 1), (300, 260)]


def words(K):
    """(H, W) uint32 as the RGBA8 frame that holds it."""
    return np.ascontiguousarray(K, np.uint32).view(np.uint8).reshape(K.shape + (4,))


def plane_of(ctx, k, p, reach, pass_static):
    ctx.hole_fill_plane(k, p, reach, pass_static)
    return ctx.download(p).view(np.uint32)[..., 0]


@pytest.mark.parametrize("w,h", SIZES)
def test_plane_equals_the_model(ctx, w, h):
    """Every crafted pattern at every reach, with and without pass_static.  fill_cases.cross_at_seams and fill_cases.seams put
    donors exactly reach and reach + 1 from the 64-pixel seams of the row pass and the band seams of the column pass."""
    p = ctx.create_frame(w, h)
    try:
        for reach in fc.REACHES:
            for name, K in fc.patterns(w, h, reach):
                k = ctx.frame_from(words(K))
                try:
                    for pass_static in (False, True):
                        got, want = plane_of(ctx, k, p, reach, pass_static), fm.plane(K, reach, pass_static)
                        assert (got == want).all(), (name, reach, pass_static, np.argwhere(got != want)[:4].tolist())
                finally:
                    ctx.destroy_frame(k)
    finally:
        ctx.destroy_frame(p)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("pads", [(3, 5), (4, 0), (1, 12)])
def test_plane_with_padded_pitches(ctx, w, h, pads):
    """Rows that start off a 16-byte boundary (the row pass's dword loads) and rows that start on one; the padding of the plane
    keeps its bytes."""
    reach = 65
    K = fc.random_keys(w, h, 50, seed=5)
    big_k, k = pitched(ctx, words(K), pads[0])
    big_p, p = pitched(ctx, np.zeros((h, w, 4), np.uint8), pads[1])
    try:
        for pass_static in (False, True):
            ctx.hole_fill_plane(k, p, reach, pass_static)
            wide = ctx.download(big_p)
            got, want = wide[:, :w].copy().view(np.uint32)[..., 0], fm.plane(K, reach, pass_static)
            assert (got == want).all(), (pads, pass_static, np.argwhere(got != want)[:4].tolist())
            assert (wide[:, w:] == 0x5A).all()
    finally:
        ctx.destroy_frame(big_k)
        ctx.destroy_frame(big_p)


def test_invalid_arguments_launch_nothing(ctx):
    K = fc.random_keys(40, 30, 3, seed=1)
    k, p, small = ctx.frame_from(words(K)), ctx.frame_from(np.full((30, 40, 4), 7, np.uint8)), ctx.create_frame(39, 30)
    mvf = ctx.create_frame(40, 30, MV)
    try:
        fill = lambda *a: ctx.lib.lfg_hole_fill_plane(ctx.h, *a)
        ref = ctypes.byref
        assert fill(ref(k), 0, 0, ref(p)) == -1 and fill(ref(k), capi.HOLE_REACH_MAX + 1, 0, ref(p)) == -1
        assert fill(ref(k), 16, 2, ref(p)) == -1 and fill(ref(k), 16, -1, ref(p)) == -1
        assert fill(ref(k), 16, 0, ref(small)) == -1 and fill(ref(k), 16, 0, ref(mvf)) == -1
        assert fill(ref(k), 16, 0, ref(k)) == -1 and fill(None, 16, 0, ref(p)) == -1 and fill(ref(k), 16, 0, None) == -1
        odd = capi.Context.wrap(k.data + 2, 38, 30, capi.FORMAT_RGBA8, pitch=160)     # two bytes off a word
        assert fill(ref(odd), 16, 0, ref(capi.Context.wrap(p.data, 38, 30, capi.FORMAT_RGBA8, pitch=160))) == -1
        assert "lfg_hole_fill_plane" in ctx.lib.lfg_last_error(ctx.h).decode()
        assert (ctx.download(p) == 7).all()
        for bad in (0, -2, capi.HOLE_REACH_MAX + 1):
            assert ctx.lib.lfg_set_hole_reach(ctx.h, bad) == -1
        assert "lfg_set_hole_reach" in ctx.lib.lfg_last_error(ctx.h).decode()
    finally:
        for f in (k, p, small, mvf):
            ctx.destroy_frame(f)


# ---- the three calls under lfg_set_hole_reach

FACTORS = (0.5, 0.25)
REACHES = (16, 32, 255)
_scenes = {}


def scene(ctx, name):
    """(prev, curr, fwd, bwd, mask): scene B with its true field or with the GPU pyramid's vectors, or mc.moving_square with the
    GPU's full search; the mask is lfg_static_mask's at tolerance 0 (its model).  Made once."""
    if name not in _scenes:
        if name == "moving square":
            prev, curr, _ = mc.moving_square()
            fwd, bwd = gpu_vectors(ctx, prev, curr, "full"), gpu_vectors(ctx, curr, prev, "full")
        else:
            (prev, _, curr), fwd, bwd = fc.scene_fields(fm.SCENE_B)
            if name == "scene B, pyramid":
                fwd, bwd = gpu_vectors(ctx, prev, curr, "pyramid"), gpu_vectors(ctx, curr, prev, "pyramid")
        _scenes[name] = prev, curr, fwd, bwd, ov.static_mask(prev, curr, 0)
    return _scenes[name]


@pytest.fixture
def reach_restored(ctx):
    yield
    ctx.set_hole_reach(-1)
    ctx.set_generation(capi.GENERATION_INTERPOLATE)
    apply(ctx, DEFAULT)


@pytest.mark.parametrize("name", ["scene B, true field", "scene B, pyramid", "moving square"])
def test_the_three_calls_equal_the_model(ctx, reach_restored, name):
    """Each call at each reach and factor is the model's frame; at reach 16 it is also the same call with the setting off, which
    holds the kernels that read the plane to the ones that walk."""
    prev, curr, fwd, bwd, mask = scene(ctx, name)
    h, w = prev.shape[:2]
    p, c, f, b, o = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(fwd, MV), ctx.frame_from(bwd, MV), ctx.create_frame(w, h)
    mf, m = ctx.mask_from(mask)
    calls = {"compensated": lambda t: ctx.interpolate_compensated(p, c, f, o, t, 48),
             "masked": lambda t: ctx.interpolate_compensated_masked(p, c, f, m, o, t, 48),
             "bidirectional": lambda t: ctx.interpolate_compensated_bidirectional(p, c, f, b, o, t, 48, 1)}
    models = {"compensated": lambda t, r: fm.interpolate_compensated(prev, curr, fwd, t, r, 48),
              "masked": lambda t, r: fm.interpolate_masked(prev, curr, fwd, mask, t, r, 48),
              "bidirectional": lambda t, r: fm.interpolate_bidirectional(prev, curr, fwd, bwd, t, r, 48, 1)}
    try:
        for call in calls:
            for t in FACTORS:
                ctx.set_hole_reach(-1)
                calls[call](t)
                off = ctx.download(o)
                for reach in REACHES:
                    ctx.set_hole_reach(reach)
                    calls[call](t)
                    got, want = ctx.download(o), models[call](t, reach)
                    assert (got == want).all(), (call, t, reach, first_bad(got, want))
                    if reach == 16:
                        assert (got == off).all(), (call, t, first_bad(got, off))
        if name == "scene B, true field":                    # the reach shows: the frames at 16 and at 32 differ
            assert (models["compensated"](0.5, 16) != models["compensated"](0.5, 32)).any()
    finally:
        for x in (p, c, f, b, o, mf):
            ctx.destroy_frame(x)


def test_multi_equals_single_calls(ctx, reach_restored):
    prev, curr, fwd, bwd, mask = scene(ctx, "scene B, true field")
    h, w = prev.shape[:2]
    factors = [0.25, 0.5, 0.75]
    p, c, f = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(fwd, MV)
    outs = [ctx.create_frame(w, h) for _ in factors]
    try:
        ctx.set_hole_reach(64)
        ctx.interpolate_compensated_multi(p, c, f, outs, factors, 48)
        for t, o in zip(factors, outs):
            got, want = ctx.download(o), fm.interpolate_compensated(prev, curr, fwd, t, 64, 48)
            assert (got == want).all(), (t, first_bad(got, want))
    finally:
        for x in [p, c, f] + outs:
            ctx.destroy_frame(x)


def test_extrapolation_and_the_shader_ignore_the_setting(ctx, reach_restored):
    prev, curr, fwd, _, _ = scene(ctx, "scene B, true field")
    h, w = prev.shape[:2]
    p, c, f = ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(fwd, MV)
    outs = [ctx.create_frame(w, h) for _ in range(2)]
    try:
        for reach, o in zip((-1, 255), outs):
            ctx.set_hole_reach(reach)
            ctx.extrapolate_compensated(p, c, f, o, 0.5, 48)
        assert (ctx.download(outs[0]) == ctx.download(outs[1])).all()
        apply(ctx, ("pyramid", -1, "shader", capi.SEMANTICS_INTENDED))
        for reach, o in zip((-1, 255), outs):
            ctx.set_hole_reach(reach)
            ctx.interpolate_frames(p, c, o, 0.5)
        assert (ctx.download(outs[0]) == ctx.download(outs[1])).all()
        apply(ctx, ("pyramid", -1, "compensated", capi.SEMANTICS_INTENDED))
        ctx.set_generation(capi.GENERATION_EXTRAPOLATE)
        for reach, o in zip((-1, 255), outs):
            ctx.set_hole_reach(reach)
            ctx.interpolate_frames(p, c, o, 0.5)
        assert (ctx.download(outs[0]) == ctx.download(outs[1])).all()
    finally:
        for x in [p, c, f] + outs:
            ctx.destroy_frame(x)


# ---- lfg_interpolate_frames_multi, two lanes

def test_frames_multi_on_two_lanes(ctx, reach_restored):
    """Two pairs of one size and different content, one per lane, both enqueued before the one sync: each lane has a key image
    and a fill plane of its own, so each output is the CPU chain's (the pyramid's model, then the fill model)."""
    factors = [0.25, 0.5, 0.75]
    pairs = []
    for seed in (3, 4):
        (prev, _, curr), _ = fm.fast_scene(**fm.SCENE_B, seed=seed)
        pairs.append((prev, curr))
    apply(ctx, ("pyramid", -1, "compensated", capi.SEMANTICS_INTENDED))
    ctx.set_hole_reach(32)
    ctx.lanes(2)
    frames = []
    try:
        for lane, (prev, curr) in enumerate(pairs):
            ctx.lane_select(lane)
            h, w = prev.shape[:2]
            p, c = ctx.frame_from(prev), ctx.frame_from(curr)
            outs = [ctx.create_frame(w, h) for _ in factors]
            frames.append((p, c, outs))
        for _ in range(2):                                   # twice: the second round reuses both lanes' buffers
            for lane, (p, c, outs) in enumerate(frames):
                ctx.lane_select(lane)
                ctx.interpolate_frames_multi(p, c, outs, factors)
        ctx.sync()
        for (prev, curr), (p, c, outs) in zip(pairs, frames):
            mv = pm.motion_pyramid(prev, curr, 2, 16, 2)
            for t, o in zip(factors, outs):
                got, want = ctx.download(o), fm.interpolate_compensated(prev, curr, mv, t, 32, 48)
                assert (got == want).all(), (t, first_bad(got, want))
    finally:
        ctx.lane_select(0)
        for p, c, outs in frames:
            for x in [p, c] + outs:
                ctx.destroy_frame(x)
        ctx.lanes(1)


# ---- lfg_host --hole-reach

def test_host_hole_reach_matches_the_chain(tmp_path):
    """A five-frame stream of scene B's kind, wide enough for the square's four steps: every generated frame is the CPU chain's
    on the frames the host interpolates between (its own 1:1 upscale of the input), and the real frames pass through."""
    sc = dict(fm.SCENE_B, w=320)
    frames, _ = fm.fast_scene(**sc, frames=(0, 1, 2, 3, 4))
    n, (h, w) = len(frames), frames[0].shape[:2]
    info, got = host_run(tmp_path, frames, (w, h), "--semantics", "intended", "--motion", "pyramid", "--interpolator", "compensated",
                         "--hole-reach", "32")
    assert len(got) == 2 * n - 1 and info["hole_reach"] == 32
    with capi.Context(0) as c:
        ups = []
        for f in frames:
            i, u = c.frame_from(f), c.create_frame(w, h)
            c.scale(i, u)
            ups.append(c.download(u))
    differs = 0
    for k in range(1, n):
        assert (got[2 * k] == ups[k]).all(), k
        mv = pm.motion_pyramid(ups[k - 1], ups[k], 2, 16, 2)
        want = fm.interpolate_compensated(ups[k - 1], ups[k], mv, 0.5, 32, 48)
        assert (got[2 * k - 1] == want).all(), (k, first_bad(got[2 * k - 1], want))
        differs += int((want != mc.interpolate_compensated(ups[k - 1], ups[k], mv, 0.5, 48)).any())
    assert differs                                           # the option shows on this stream
