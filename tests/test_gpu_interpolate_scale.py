"""lfg_interpolate_scale against the CPU chain -- oracle.interpolate, then the float64 Lanczos model of its 2x upscale
(oracle/scale_f64.py) -- on frames that sample (tests/cases.py: sampling_scene; tests/test_sampling_scene.py holds it to
that): the fused kernel (scale_2x_kernel<true>, lfg_scale_last_kernel() == 2) at the sizes chosen around the 2x kernel's
seams, at full size on every pixel, on pitched frames, on every route that leaves it, and on three lanes.  Every case also
holds lfg_interpolate itself to the oracle byte for byte, under both semantics."""
import numpy as np
import pytest

from linux_fg_amd import capi
from oracle import scale_f64 as f64
from tests import cases
from tests.gpu_kit import assert_matches_f64, ctx, first_bad, pitched, seam_rows, three_lanes
from tests.test_gpu_dispatch import SIZES as DISPATCH_SIZES

pytestmark = pytest.mark.gpu

SEMANTICS = (capi.SEMANTICS_REFERENCE, capi.SEMANTICS_INTENDED)
POISON = 0xA5


@pytest.fixture(autouse=True)
def _settings_restored(ctx):
    yield
    ctx.set_semantics(capi.SEMANTICS_REFERENCE)
    ctx.set_fused_interpolate_scale(False)


def poison(ctx, frame):
    ctx.upload(frame, np.full((frame.height, frame.width, 4), POISON, np.uint8))


def upload_scene(ctx, prev, curr, mv):
    return ctx.frame_from(prev), ctx.frame_from(curr), ctx.frame_from(mv, capi.FORMAT_MV_S8X2)


def mid_of(oracle, prev, curr, mv, t, sem):
    return oracle.interpolate(prev, curr, mv.astype(np.float32), t, semantics=sem)


def interpolate_scale(ctx, p, c, m, out, t, fuse, kernel, what):
    """One poisoned call; the bytes it left."""
    poison(ctx, out)
    ctx.set_fused_interpolate_scale(fuse)
    ctx.interpolate_scale(p, c, m, out, t)
    assert ctx.scale_last_kernel() == kernel, f"{what}: fused flag {fuse}, kernel {ctx.scale_last_kernel()}, expected {kernel}"
    return ctx.download(out)


def staged_call(ctx, oracle, p, c, m, mid, out, t, mid_want, kernel, what):
    """lfg_interpolate into `mid` (byte for byte the oracle's frame), then lfg_scale of it into `out`: out's bytes."""
    poison(ctx, mid)
    ctx.interpolate(p, c, m, mid, t)
    got = ctx.download(mid)
    assert (got == mid_want).all(), f"{what}: lfg_interpolate against the oracle: {first_bad(got, mid_want)}"
    poison(ctx, out)
    ctx.scale(mid, out)
    assert ctx.scale_last_kernel() == kernel, f"{what}: lfg_scale took kernel {ctx.scale_last_kernel()}, expected {kernel}"
    return ctx.download(out)


def assert_model(got, mid_want, what, band=None):
    """`got` against the float64 model of mid_want's 2x upscale, every pixel (in bands of `band` output rows: bounded memory);
    for outputs of 4096 bytes and more the near-ties, where the model decides nothing, are at most 1 % of the bytes."""
    h, w = mid_want.shape[:2]
    W, H = 2 * w, 2 * h
    ties = 0
    for y0 in range(0, H, band or H):
        y1 = min(y0 + (band or H), H)
        ties += assert_matches_f64(got[y0:y1], f64.scale_f64(mid_want, W, H, roi=(0, y0, W, y1)), what=f"{what} rows {y0}..{y1}")
    print(f"near-tie share {what}: {ties / got.size:.3%}")
    if got.size >= 4096:
        assert ties <= 0.01 * got.size, f"{what}: {ties} near-ties in {got.size} bytes"


def check_2x(ctx, oracle, scene, t, sem, what, band=None):
    """The whole comparison of one scene at one factor under one semantics, out exactly 2x the inputs."""
    prev, curr, mv = scene
    h, w = prev.shape[:2]
    what = f"{what} {w}x{h} t={t} semantics {sem}"
    mid_want = mid_of(oracle, prev, curr, mv, t, sem)
    p, c, m = upload_scene(ctx, prev, curr, mv)
    mid, out = ctx.create_frame(w, h), ctx.create_frame(2 * w, 2 * h)
    try:
        ctx.set_semantics(sem)
        staged = staged_call(ctx, oracle, p, c, m, mid, out, t, mid_want, 1, what)
        default = interpolate_scale(ctx, p, c, m, out, t, False, 1, what)
        assert (default == staged).all(), f"{what}: default against staged: {first_bad(default, staged)}"
        del default
        fused = interpolate_scale(ctx, p, c, m, out, t, True, 2, what)
        assert (fused == staged).all(), f"{what}: fused against staged: {first_bad(fused, staged)}"
        del staged
    finally:
        for f in (p, c, m, mid, out):
            ctx.destroy_frame(f)
    assert_model(fused, mid_want, what, band)


# ---- 1. the sweep

# three shapes of the sweep with a second workgroup per row (more than 480 columns) or more than one strip per XCD (bands of
# 17 rows at 135 and 136): the factors at which a sample is all prev or all curr, and one more that is inexact in fp32
MORE_FACTORS = {(962, 135): (0.0, 1.0, 0.9), (482, 35): (0.0, 1.0, 0.9), (6, 136): (0.0, 1.0, 0.9)}
assert set(MORE_FACTORS) <= set(f64.sweep_2x_shapes())


def impulse_scene(w, h):
    """prev = curr = the scale tests' impulses, seam-row impulses included, so that the generated frame carries them where the
    vectors are zero: everywhere but on the seam rows themselves, which take the sampling scene's vectors."""
    rows = seam_rows(h)
    imp = f64.contents(w, h, seed=1000 * w + h, seam_rows=rows)["impulses"]
    mv = np.zeros((h, w, 2), np.int8)
    mv[rows] = cases.sampling_scene_of(w, h)[2][rows]
    return imp, imp.copy(), mv


@pytest.mark.parametrize("sem", SEMANTICS)
@pytest.mark.parametrize("wh", f64.sweep_2x_shapes(), ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_sweep_against_the_chain(ctx, oracle, wh, sem):
    """The fused kernel at input widths around its 120 owned columns per wave and 480 per workgroup and heights from 1 to
    the strip lengths, on the scene that samples: every row a strip re-reads and every wave seam carries vectors."""
    scene = cases.sampling_scene_of(*wh)
    for t in cases.SAMPLING_FACTORS + MORE_FACTORS.get(wh, ()):
        check_2x(ctx, oracle, scene, t, sem, "sweep")
    check_2x(ctx, oracle, impulse_scene(*wh), 0.5, sem, "sweep, impulses")


# ---- 2. full size, every pixel

@pytest.mark.parametrize("sem,t", [(capi.SEMANTICS_REFERENCE, 0.3), (capi.SEMANTICS_REFERENCE, 0.5), (capi.SEMANTICS_INTENDED, 0.3)])
def test_1080p_to_4k_every_pixel(ctx, oracle, sem, t):
    check_2x(ctx, oracle, cases.sampling_scene_of(1920, 1080), t, sem, "1080p -> 4K", band=540)


def test_4k_to_8k_every_pixel(ctx, oracle):
    check_2x(ctx, oracle, cases.sampling_scene_of(3840, 2160), 0.3, capi.SEMANTICS_INTENDED, "4K -> 8K", band=540)


# ---- 3. pitched frames

@pytest.mark.parametrize("sem", SEMANTICS)
@pytest.mark.parametrize("w,h", [(242, 35), (64, 36)])
def test_pitched_frames(ctx, oracle, w, h, sem):
    """prev, curr and the vectors with rows 1, 3 and 5 pixels longer than the image; the output's rows a multiple of 16 bytes
    apart (the fused kernel) or 8 mod 16 (the flag is on, but the fused kernel stores 16 bytes at a time: the two stages, with
    the generic scale kernel).  No padding is written."""
    t = 0.3
    prev, curr, mv = cases.sampling_scene_of(w, h)
    mid_want = mid_of(oracle, prev, curr, mv, t, sem)
    (bp, vp), (bc, vc) = pitched(ctx, prev, 1), pitched(ctx, curr, 3)
    bm, vm = pitched(ctx, mv, 5, capi.FORMAT_MV_S8X2)
    mid, plain = ctx.create_frame(w, h), ctx.create_frame(2 * w, 2 * h)
    ctx.set_semantics(sem)
    staged = staged_call(ctx, oracle, vp, vc, vm, mid, plain, t, mid_want, 1, f"pitched {w}x{h}")
    for out_pad, kernel in ((4, 2), (2, 0)):
        what = f"pitched {w}x{h} -> +{out_pad} semantics {sem}"
        assert ((2 * w + out_pad) * 4) % 16 == (0 if kernel else 8)
        bo, vo = pitched(ctx, np.full((2 * h, 2 * w, 4), POISON, np.uint8), out_pad)
        ctx.set_fused_interpolate_scale(True)
        ctx.interpolate_scale(vp, vc, vm, vo, t)
        assert ctx.scale_last_kernel() == kernel, what
        full = ctx.download(bo)
        assert (full[:, 2 * w:] == 0x5A).all(), what
        if kernel:
            assert (full[:, :2 * w] == staged).all(), f"{what}: {first_bad(full[:, :2 * w], staged)}"
        assert_model(full[:, :2 * w], mid_want, what)
        ctx.destroy_frame(bo)
    for big, host in ((bp, prev), (bc, curr), (bm, mv)):
        full = ctx.download(big)
        assert (full[:, w:] == 0x5A).all() and (full[:, :w] == host).all()
    for f in (bp, bc, bm, mid, plain):
        ctx.destroy_frame(f)


# ---- 4. routing with the flag on: every reason for leaving the fused kernel, and the one large view that stays on it

def routed(ctx, oracle, scene, out_wh, sem, t, kernel, what, views=None, out_view=None):
    """With the flag on, lfg_interpolate_scale of `scene` (or of `views` of it) into a frame of out_wh (or into out_view) takes
    `kernel`, and gives, byte for byte, what lfg_interpolate and lfg_scale give on the same frames.  Returns the bytes."""
    prev, curr, mv = scene
    h, w = prev.shape[:2]
    mid_want = mid_of(oracle, prev, curr, mv, t, sem)
    own = [] if views else list(upload_scene(ctx, prev, curr, mv))
    p, c, m = views or own
    mid = ctx.create_frame(w, h)
    out = out_view or ctx.create_frame(*out_wh)
    own += [mid] if out_view else [mid, out]
    try:
        ctx.set_semantics(sem)
        staged = staged_call(ctx, oracle, p, c, m, mid, out, t, mid_want, min(kernel, 1), what)
        got = interpolate_scale(ctx, p, c, m, out, t, True, kernel, what)
        assert (got == staged).all(), f"{what}: {first_bad(got, staged)}"
    finally:
        for f in own:
            ctx.destroy_frame(f)
    return got, mid_want


@pytest.mark.parametrize("sem", SEMANTICS)
def test_odd_width_takes_the_generic_kernel(ctx, oracle, sem):
    got, mid_want = routed(ctx, oracle, cases.sampling_scene_of(121, 40), (242, 80), sem, 0.3, 0, "121x40 -> 242x80")
    assert_model(got, mid_want, f"121x40 -> 242x80 semantics {sem}")


@pytest.mark.parametrize("sem", SEMANTICS)
@pytest.mark.parametrize("out_wh", [(200, 90), (240, 81), (120, 40)])
def test_other_ratios_take_the_generic_kernel(ctx, oracle, out_wh, sem):
    """1.67 x 2.25, 2 x 2.025 and 1 x 1: against the float64 model of the same resize."""
    w, h = 120, 40
    got, mid_want = routed(ctx, oracle, cases.sampling_scene_of(w, h), out_wh, sem, 0.3, 0, f"{w}x{h} -> {out_wh}")
    ties = assert_matches_f64(got, f64.scale_f64(mid_want, *out_wh), what=f"{w}x{h} -> {out_wh} semantics {sem}")
    assert ties <= 0.01 * got.size


@pytest.mark.parametrize("sem", SEMANTICS)
def test_output_4_bytes_into_an_allocation_takes_the_generic_kernel(ctx, oracle, sem):
    """Rows a multiple of 16 bytes apart, but the base is not: the 2x kernels store 16 bytes at a time."""
    w, h = 120, 40
    alloc = ctx.create_frame(2 * w, 2 * h + 1)
    poison(ctx, alloc)
    view = capi.Context.wrap(alloc.data + 4, 2 * w, 2 * h, capi.FORMAT_RGBA8, pitch=8 * w)
    got, mid_want = routed(ctx, oracle, cases.sampling_scene_of(w, h), None, sem, 0.3, 0, "output base + 4", out_view=view)
    assert_model(got, mid_want, f"output base + 4, semantics {sem}")
    raw = ctx.download(alloc).reshape(-1)
    assert (raw[:4] == POISON).all() and (raw[4 + got.size:] == POISON).all()
    ctx.destroy_frame(alloc)


@pytest.mark.parametrize("big,kernel", [("prev", 1), ("curr", 1), ("out", 0), ("mv", 2)])
def test_views_of_2_gib_and_more(ctx, oracle, big, kernel):
    """The fused kernel addresses prev, curr and out with 32-bit byte offsets: a view of one of them that spans 2 GiB or more
    (rows tens of MB apart) sends the call through the two stages -- with the exact-2x scale kernel, whose own input is the
    context's frame, or the generic one for such an output.  The vectors are indexed with size_t: the fused kernel stays."""
    w, h = 64, 40
    sem, t = capi.SEMANTICS_INTENDED, 0.3
    scene = cases.sampling_scene_of(w, h)
    alloc = ctx.create_frame(24000, 24000)                        # 2.304e9 bytes
    frames = dict(zip(("prev", "curr", "mv"), upload_scene(ctx, *scene)))
    out_view = None
    if big == "out":
        out_view = capi.Context.wrap(alloc.data, 2 * w, 2 * h, capi.FORMAT_RGBA8, pitch=27_000_000)   # a multiple of 16; 79 * pitch + 512 < 2.304e9
        assert out_view.height * out_view.pitch >= 2 ** 31
    else:
        fmt = capi.FORMAT_MV_S8X2 if big == "mv" else capi.FORMAT_RGBA8
        view = capi.Context.wrap(alloc.data, w, h, fmt, pitch=57_600_000)                               # 39 * pitch + 256 < 2.304e9
        assert view.height * view.pitch >= 2 ** 31
        ctx.upload(view, scene[("prev", "curr", "mv").index(big)])
        ctx.destroy_frame(frames[big])
        frames[big] = view
    views = [frames["prev"], frames["curr"], frames["mv"]]
    try:
        got, mid_want = routed(ctx, oracle, scene, (2 * w, 2 * h), sem, t, kernel, f"2 GiB {big}", views=views, out_view=out_view)
    finally:
        for name, f in frames.items():
            if name != big:
                ctx.destroy_frame(f)
        ctx.destroy_frame(alloc)
    assert_model(got, mid_want, f"2 GiB {big}")


# ---- 5. three lanes

# the dispatch tests' sizes with even widths, then enough further ones for more than 14 axis lengths (each size brings two
# axis tables, w -> 2w and h -> 2h, and two uv tables): tables are trimmed while kernels that read older ones are queued
LANE_SIZES = [(w + w % 2, h) for w, h in DISPATCH_SIZES] + [(482, 35), (122, 9), (240, 18), (96, 54), (250, 70), (118, 7),
                                                             (962, 16), (6, 136), (124, 34)]
LANE_FACTORS = (0.3, 0.5, 0.9)
assert len({n for wh in LANE_SIZES for n in wh}) > 14


def test_three_lanes_equal_one_lane_and_the_chain(ctx, oracle):
    """Pair k on lane k % 3 under semantics k % 2, everything enqueued before the one sync, with the flag on (the fused
    kernel) and off (each lane's own temporary frame): every output is what one lane gave, which is the chain."""
    scenes = [cases.sampling_scene(w, h, 300 + k) for k, (w, h) in enumerate(LANE_SIZES)]
    setting = [(SEMANTICS[k % 2], LANE_FACTORS[k % 3]) for k in range(len(scenes))]
    alone = []
    for k, (scene, (sem, t)) in enumerate(zip(scenes, setting)):
        got, mid_want = routed(ctx, oracle, scene, tuple(2 * n for n in LANE_SIZES[k]), sem, t, 2, f"one lane, pair {k}")
        assert_model(got, mid_want, f"one lane, pair {k} {LANE_SIZES[k]}")
        alone.append(got)
    for fuse in (True, False):
        def enqueue(k, p, c, m, out):                # the call alone: an upload would wait for every lane
            ctx.set_semantics(setting[k][0])
            ctx.interpolate_scale(p, c, m, out, setting[k][1])
            assert ctx.scale_last_kernel() == (2 if fuse else 1)
            return p, c, m, out
        frames = []
        for (w, h), scene in zip(LANE_SIZES, scenes):
            frames.append(upload_scene(ctx, *scene) + (ctx.create_frame(2 * w, 2 * h),))
            poison(ctx, frames[-1][-1])
        ctx.set_fused_interpolate_scale(fuse)
        three_lanes(ctx, frames, enqueue, alone)
