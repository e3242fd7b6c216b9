"""The kernels held to what the reference's own shaders gave when their text ran on the CPU (oracle/ref_recipe.py), on a real
MI355X.  Reads the two fixture files only -- tests/golden/ref_shaders.npz, written from the executed shaders, and
tests/golden/golden_small.npz, which tests/test_reference_shaders.py holds to them -- never the reference and never
oracle/_ref.

Bars: lfg_scale within +-1 LSB of the shader's bytes; lfg_motion equal to the shader's vectors; lfg_interpolate and
lfg_interpolate_frames equal to the shader's bytes outside the fixture's mask and equal to the ORACLE inside it.  The mask is
where interpolate.comp's texture() on the vector image has a non-zero fractional weight in fp32 (oracle.inexact_centres); the
product reads the texel there, as choice (8) of lfg_oracle.c says a device's fixed-point filter does, and the second half of
the bar records that it follows (8) and not the fp32 idealisation."""
import os

import numpy as np
import pytest

import oracle
from linux_fg_amd import capi
from tests.gpu_kit import DEFAULT, apply, ctx, first_bad, pitched  # noqa: F401  (ctx is this module's fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def shaders():
    return np.load(os.path.join(GOLDEN, "ref_shaders.npz"))


@pytest.fixture(scope="module")
def small():
    return np.load(os.path.join(GOLDEN, "golden_small.npz"))


def run(ctx, call, inputs, out_shape, out_fmt=capi.FORMAT_RGBA8):
    """call(*input frames, output frame) on fresh frames; `inputs` are (array, format) pairs."""
    frames = [ctx.frame_from(a, f) for a, f in inputs]
    out = ctx.create_frame(out_shape[1], out_shape[0], out_fmt)
    try:
        call(*frames, out)
        return ctx.download(out)
    finally:
        for f in frames + [out]:
            ctx.destroy_frame(f)


def scaled(ctx, src, w, h):
    return run(ctx, ctx.scale, [(src, capi.FORMAT_RGBA8)], (h, w))


def vectors(ctx, prev, curr, bs, radius):
    return run(ctx, lambda p, c, m: ctx.motion(p, c, m, bs, radius), [(prev, capi.FORMAT_RGBA8), (curr, capi.FORMAT_RGBA8)],
               prev.shape[:2], capi.FORMAT_MV_S8X2)


def assert_shader_outside_oracle_inside(got, shader, oracle_bytes, mask, what):
    outside = np.where(mask[..., None], shader, got)
    assert (outside == shader).all(), f"{what}: outside the mask {first_bad(outside, shader)}"
    inside = np.where(mask[..., None], got, oracle_bytes)
    assert (inside == oracle_bytes).all(), f"{what}: inside the mask {first_bad(inside, oracle_bytes)}"


@pytest.mark.parametrize("w,h", [(13, 8), (33, 19)], ids=["down", "ragged-up"])
def test_scale_within_one_lsb_of_the_shader(ctx, shaders, w, h):
    got, want = scaled(ctx, shaders["scale_in"], w, h), shaders[f"scale_{w}x{h}"]
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert d.max() <= 1, f"max |diff| = {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"


def test_scale_of_golden_small_within_one_lsb_of_the_shader(ctx, small):
    for src, w, h, name in (("prev_in", 128, 72, "prev_up"), ("curr_in", 128, 72, "curr_up"), ("curr_in", 53, 41, "curr_53x41")):
        d = np.abs(scaled(ctx, small[src], w, h).astype(np.int16) - small[name].astype(np.int16))
        assert d.max() <= 1, (name, int(d.max()))


@pytest.mark.parametrize("w,bs,radius", [(64, 8, 16.0), (100, 8, 16.0), (100, 4, 3.0)])
def test_motion_equals_the_shader(ctx, shaders, w, bs, radius):
    """Pairs with a flat patch (every candidate ties) and an occluder of fresh noise (no candidate matches)."""
    want = shaders[f"mv_{w}_b{bs}_r{int(radius)}"]
    got = vectors(ctx, shaders[f"prev_{w}"], shaders[f"curr_{w}"], bs, radius)
    assert (got == want).all(), first_bad(got, want)


def test_motion_of_golden_small_equals_the_shader(ctx, small):
    got = vectors(ctx, small["prev_up"], small["curr_up"], 8, 16.0)
    assert (got == small["mv"]).all(), first_bad(got, small["mv"])
    got = vectors(ctx, small["prev_in"], small["curr_in"], 4, 3.0)
    assert (got == small["mv_b4_r3"]).all(), first_bad(got, small["mv_b4_r3"])


@pytest.mark.parametrize("w", [64, 100])
@pytest.mark.parametrize("t", [50, 30])
def test_interpolate_equals_the_shader_outside_the_mask_and_the_oracle_inside(ctx, shaders, w, t):
    """lfg_interpolate on the shader's own vectors, and lfg_interpolate_frames on the same pair (default settings: the full
    search at (8, 16), the shader's interpolation, the reference's semantics), which has to find those vectors first.  At
    64 x 32 the mask is empty: the shader's bytes everywhere."""
    prev, curr, mv, shader = shaders[f"prev_{w}"], shaders[f"curr_{w}"], shaders[f"mv_{w}_b8_r16"], shaders[f"interp_{w}_{t}"]
    mask = shaders["mask_100"] if w == 100 else np.zeros(mv.shape[:2], bool)
    want = oracle.interpolate(prev, curr, mv.astype(np.float32), t / 100)
    if w == 100 and t == 50:
        assert ((want != shader).any(-1) & mask).any()           # the fixture keeps a pixel on which (8) and the shader part
    frames = [(prev, capi.FORMAT_RGBA8), (curr, capi.FORMAT_RGBA8)]
    got = run(ctx, lambda p, c, m, o: ctx.interpolate(p, c, m, o, t / 100), frames + [(mv, capi.FORMAT_MV_S8X2)], prev.shape[:2])
    assert_shader_outside_oracle_inside(got, shader, want, mask, "lfg_interpolate")
    apply(ctx, DEFAULT)
    got = run(ctx, lambda p, c, o: ctx.interpolate_frames(p, c, o, t / 100), frames, prev.shape[:2])
    assert_shader_outside_oracle_inside(got, shader, want, mask, "lfg_interpolate_frames")


def test_interpolate_of_golden_small_equals_the_shader(ctx, small):
    frames = [(small["prev_up"], capi.FORMAT_RGBA8), (small["curr_up"], capi.FORMAT_RGBA8), (small["mv"], capi.FORMAT_MV_S8X2)]
    for t in (25, 50, 75):
        got = run(ctx, lambda p, c, m, o: ctx.interpolate(p, c, m, o, t / 100), frames, small["prev_up"].shape[:2])
        assert (got == small[f"interp_{t}"]).all(), (t, first_bad(got, small[f"interp_{t}"]))


def test_padded_pitch(ctx, shaders):
    """The 100 x 36 pair as the left part of wider frames, every row pitch padded by a different odd number of pixels: the
    vectors and the generated frame are the shader's (outside the mask), and the padding is never written."""
    prev, curr, mask = shaders["prev_100"], shaders["curr_100"], shaders["mask_100"]
    h, w = prev.shape[:2]
    bp, vp = pitched(ctx, prev, 3)
    bc, vc = pitched(ctx, curr, 5)
    bm, vm = pitched(ctx, np.zeros((h, w, 2), np.int8), 7, capi.FORMAT_MV_S8X2)
    bo, vo = pitched(ctx, np.zeros((h, w, 4), np.uint8), 1)
    try:
        ctx.motion(vp, vc, vm, 8, 16.0)
        ctx.interpolate(vp, vc, vm, vo, 0.5)
        mv, out = ctx.download(bm), ctx.download(bo)
    finally:
        for f in (bp, bc, bm, bo):
            ctx.destroy_frame(f)
    assert (mv[:, w:] == 0x5A).all() and (out[:, w:] == 0x5A).all()
    assert (mv[:, :w] == shaders["mv_100_b8_r16"]).all(), first_bad(mv[:, :w], shaders["mv_100_b8_r16"])
    want = oracle.interpolate(prev, curr, shaders["mv_100_b8_r16"].astype(np.float32), 0.5)
    assert_shader_outside_oracle_inside(out[:, :w], shaders["interp_100_50"], want, mask, "pitched lfg_interpolate")
