"""Frame comparison on the GPU: lfg_frame_diff against the CPU model (tests/diff_model.py) in exact integers -- every seam size,
four masks, both load paths, regions of interest, sums beyond 32 bits, accumulation, three lanes, argument checks -- then the
measure on the interpolators' existing exactness claims, and lfg_host --evaluate against the CPU chain (tests/cases.py)."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

from linux_fg_amd import capi, synth
from tests import cases
from tests import diff_model as dm
from tests.gpu_kit import DEFAULT, HOST, apply, ctx, pitched, three_lanes
from tests.test_diff_model import INT_KEYS, SEAM_SIZES

pytestmark = pytest.mark.gpu

RECORD_TEXELS = ctypes.sizeof(capi.FrameDiffStats) // 4


def poisoned_record(ctx):
    r = ctx.create_diff_record()
    ctx.upload(r, np.full((1, RECORD_TEXELS, 4), 0xFF, np.uint8))
    return r


def check_against_the_model(ctx, a, b, fa, fb, what, masks=dm.MASKS):
    """lfg_frame_diff(fa, fb) under every mask, twice into one poisoned record: both results are the model's of (a, b)."""
    r = poisoned_record(ctx)
    try:
        for mask in masks:
            want = dm.frame_diff(a, b, mask)
            ctx.frame_diff(fa, fb, r, mask)
            first = ctx.read_diff_record(r)
            ctx.frame_diff(fa, fb, r, mask)                   # into the same record: it writes, it does not accumulate
            again = ctx.read_diff_record(r)
            assert first == want, f"{what} mask {mask:#x}: {describe(first, want)}"
            assert again == want, f"{what} mask {mask:#x}, second call: {describe(again, want)}"
    finally:
        ctx.destroy_frame(r)


def describe(got, want):
    bins = [(k, g, e) for k, (g, e) in enumerate(zip(got[2], want[2])) if g != e]
    return f"pixels {got[0]} / {want[0]}, sse {got[1]} / {want[1]}, {len(bins)} bins differ, first (bin, got, model) {bins[:4]}"


# ---- 1. equals the model exactly: the four-pixel item, the wave, the workgroup's 1,024 items and the grid-stride tail

@pytest.mark.parametrize("w,h", SEAM_SIZES + [(1920, 1080)])
def test_equals_the_model(ctx, w, h):
    a, b = dm.graded_of(w, h)
    fa, fb = ctx.frame_from(a), ctx.frame_from(b)
    try:
        check_against_the_model(ctx, a, b, fa, fb, f"{w}x{h}")
    finally:
        ctx.destroy_frame(fa)
        ctx.destroy_frame(fb)


# ---- 2. both load paths

def pads_to_16(w):
    """Two different pads that make both row pitches multiples of 16, so that the 16-byte path runs at any width."""
    first = (-w) % 4 or 4
    return first, first + 4


@pytest.mark.parametrize("pads", [(3, 5), (4, 8), "16"], ids=lambda p: f"pads-{p}")
@pytest.mark.parametrize("w,h", SEAM_SIZES)
def test_pitched(ctx, w, h, pads):
    pad_a, pad_b = pads_to_16(w) if pads == "16" else pads
    a, b = dm.graded_of(w, h)
    big_a, fa = pitched(ctx, a, pad_a)
    big_b, fb = pitched(ctx, b, pad_b)
    if pads == "16":
        assert fa.pitch % 16 == 0 and fb.pitch % 16 == 0 and fa.data % 16 == 0 and fb.data % 16 == 0
    try:
        check_against_the_model(ctx, a, b, fa, fb, f"pitched {w}x{h} pads {pad_a}, {pad_b}", masks=(0xF, 0x5))
    finally:
        ctx.destroy_frame(big_a)
        ctx.destroy_frame(big_b)


@pytest.mark.parametrize("w,h", [(64, 4), (65, 9), (257, 131)])
def test_base_four_bytes_into_an_aligned_allocation(ctx, w, h):
    """Pitches that are multiples of 16 under a base that is not: the dword path, whatever the pitch says."""
    a, b = dm.graded_of(w, h)
    pad = pads_to_16(w + 1)[0]                                # (w + 1 + pad) * 4 is a multiple of 16
    wide_a, wide_b = np.full((h, w + 1 + pad, 4), 0x5A, np.uint8), np.full((h, w + 1 + pad, 4), 0x5A, np.uint8)
    wide_a[:, 1:w + 1], wide_b[:, 1:w + 1] = a, b
    big_a, big_b = ctx.frame_from(wide_a), ctx.frame_from(wide_b)
    fa = capi.Context.wrap(big_a.data + 4, w, h, pitch=big_a.pitch)
    fb = capi.Context.wrap(big_b.data + 4, w, h, pitch=big_b.pitch)
    aligned_b = capi.Context.wrap(big_b.data, w, h, pitch=big_b.pitch)           # columns 0 .. w - 1 of the wide frame
    assert fa.pitch % 16 == 0 and fa.data % 16 == 4
    try:
        check_against_the_model(ctx, a, b, fa, fb, f"shifted base {w}x{h}", masks=(0xF,))
        check_against_the_model(ctx, a, wide_b[:, :w], fa, aligned_b, f"one base shifted {w}x{h}", masks=(0x7,))
    finally:
        ctx.destroy_frame(big_a)
        ctx.destroy_frame(big_b)


def test_region_of_interest(ctx):
    (a, b), (w, h, x, y) = dm.graded_of(200, 120), (65, 9, 7, 3)
    fa, fb = ctx.frame_from(a), ctx.frame_from(b)
    try:
        for x0 in (x, 8):                                     # 8: a window whose base and pitch are multiples of 16
            va = capi.Context.wrap(fa.data + (y * 200 + x0) * 4, w, h, pitch=fa.pitch)
            vb = capi.Context.wrap(fb.data + (y * 200 + x0) * 4, w, h, pitch=fb.pitch)
            check_against_the_model(ctx, a[y:y + h, x0:x0 + w], b[y:y + h, x0:x0 + w], va, vb, f"window at ({x0}, {y})")
        assert (ctx.download(fa) == a).all() and (ctx.download(fb) == b).all()
    finally:
        ctx.destroy_frame(fa)
        ctx.destroy_frame(fb)


# ---- 3. sums beyond 32 bits

def test_sums_beyond_32_bits(ctx):
    w, h = 3840, 2160
    fa, fb = ctx.create_frame(w, h), ctx.create_frame(w, h)
    r = poisoned_record(ctx)
    try:
        ctx.upload(fa, np.zeros((h, w, 4), np.uint8))
        ctx.upload(fb, np.full((h, w, 4), 255, np.uint8))
        ctx.frame_diff(fa, fb, r)
        assert ctx.read_diff_record(r) == (8_294_400, (539_343_360_000,) * 4, (0,) * 255 + (8_294_400,))
        ctx.frame_diff(fb, fb, r)
        assert ctx.read_diff_record(r) == (8_294_400, (0,) * 4, (8_294_400,) + (0,) * 255)
    finally:
        for f in (fa, fb, r):
            ctx.destroy_frame(f)


# ---- 4. accumulate

def test_accumulate(ctx):
    sizes = [(200, 120), (63, 5), (1, 1)]
    pairs = [dm.graded(w, h, 50 + k) for k, (w, h) in enumerate(sizes)]
    frames = [(ctx.frame_from(a), ctx.frame_from(b)) for a, b in pairs]
    r = poisoned_record(ctx)
    try:
        for mask in (0xF, 0x5):
            models = [dm.frame_diff(a, b, mask) for a, b in pairs]
            for k, (fa, fb) in enumerate(frames):             # no host wait between them
                ctx.frame_diff(fa, fb, r, mask, accumulate=k > 0)
            got = ctx.read_diff_record(r)
            want = dm.add(dm.add(models[0], models[1]), models[2])
            assert got == want, describe(got, want)
            assert got[0] == sum(w * h for w, h in sizes)
            ctx.frame_diff(*frames[1], r, mask)               # accumulate 0 on a record that holds something
            assert ctx.read_diff_record(r) == models[1]
            ctx.frame_diff(*frames[1], r, mask, accumulate=True)
            assert ctx.read_diff_record(r) == dm.add(models[1], models[1])
    finally:
        for f in [r] + [f for pair in frames for f in pair]:
            ctx.destroy_frame(f)


# ---- 5. three lanes

LANE_SIZES = [(200, 120), (64, 36), (33, 17), (1, 1), (130, 90), (64, 4), (257, 131), (7, 5), (1025, 3)]


def test_three_lanes(ctx):
    inputs = [dm.graded(w, h, 80 + k) for k, (w, h) in enumerate(LANE_SIZES)]
    masks = [dm.MASKS[k % len(dm.MASKS)] for k in range(len(inputs))]

    def enqueue(i, a, b):
        fa, fb, r = ctx.frame_from(a), ctx.frame_from(b), poisoned_record(ctx)
        ctx.frame_diff(fa, fb, r, masks[i])
        return fa, fb, r

    alone = []
    for i, (a, b) in enumerate(inputs):
        fs = enqueue(i, a, b)
        alone.append(ctx.download(fs[-1]))
        assert ctx.read_diff_record(fs[-1]) == dm.frame_diff(a, b, masks[i])
        for f in fs:
            ctx.destroy_frame(f)
    three_lanes(ctx, inputs, enqueue, alone)


# ---- 6. validation launches nothing

def test_invalid_arguments_launch_nothing(ctx):
    lib, B = ctx.lib, ctypes.byref
    w, h = 40, 25
    a, b = dm.graded_of(w, h)
    fa, fb = ctx.frame_from(a), ctx.frame_from(b)
    mv = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    small, short = ctx.create_frame(w - 1, h), ctx.create_frame(w, h - 1)
    wide = ctx.create_frame(w + 1, h)
    odd = capi.Context.wrap(wide.data, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 2)
    shifted = capi.Context.wrap(wide.data + 2, w, h, capi.FORMAT_RGBA8, pitch=w * 4 + 4)
    empty = capi.Frame()
    r = poisoned_record(ctx)
    rec = ctypes.c_void_p(r.data)

    def diff(x, y, mask=0xF, accumulate=0, stats=rec):
        return lib.lfg_frame_diff(ctx.h, x and B(x), y and B(y), mask, accumulate, stats)

    bad = [
        diff(None, fb), diff(fa, None), diff(empty, fb), diff(fa, empty), diff(fa, fb, stats=None),      # NULL pointers, no frame
        diff(fa, fb, stats=ctypes.c_void_p(r.data + 4)),                                                 # not 8-byte aligned
        diff(mv, fb), diff(fa, mv), diff(mv, mv),                                                        # wrong format
        diff(small, fb), diff(fa, small), diff(fa, short), diff(short, fb),                              # differing sizes
        diff(odd, fb), diff(fa, odd), diff(shifted, fb), diff(fa, shifted),                              # pitch, alignment
        diff(fa, fb, 0), diff(fa, fb, 16), diff(fa, fb, 0xFFFFFFFF),                                     # the mask
        diff(fa, fb, accumulate=2), diff(fa, fb, accumulate=-1),                                         # accumulate
    ]
    assert all(rc == -1 for rc in bad), bad                   # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_frame_diff(None, B(fa), B(fb), 0xF, 0, rec) == -1
    ctx.sync()
    assert (ctx.download(r) == 0xFF).all()                    # the record keeps its poison
    assert (ctx.download(fa) == a).all() and (ctx.download(fb) == b).all()
    # the valid calls next to the bad ones work; the same frame twice is valid
    ctx.frame_diff(fa, fb, r)
    assert ctx.read_diff_record(r) == dm.frame_diff(a, b, 0xF)
    ctx.frame_diff(fa, fa, r, 0x1)
    assert ctx.read_diff_record(r) == (w * h, (0,) * 4, (w * h,) + (0,) * 255)
    ctx.frame_diff(fa, fb, r, 0x8, accumulate=True)
    assert ctx.read_diff_record(r) == dm.add(dm.frame_diff(a, a, 0x1), dm.frame_diff(a, b, 0x8))
    overlapping = capi.Context.wrap(fa.data + w * 4, w, h - 1)                     # rows 1 .. h - 1 against rows 0 .. h - 2
    upper = capi.Context.wrap(fa.data, w, h - 1)
    ctx.frame_diff(upper, overlapping, r)
    assert ctx.read_diff_record(r) == dm.frame_diff(a[:-1], a[1:], 0xF)
    assert (ctx.download(fa) == a).all() and (ctx.download(fb) == b).all()
    for f in (fa, fb, mv, small, short, wide, r):
        ctx.destroy_frame(f)


# ---- 7. the measure agrees with the existing exactness claims: compared on the device

@pytest.mark.parametrize("setting", [("full", -1, "shader", 0), ("full", 1, "compensated", 1), ("pyramid", -1, "compensated", 1)],
                         ids=lambda s: "-".join(str(v) for v in s))
def test_generated_frames_differ_nowhere_from_the_chain(ctx, setting):
    prev, curr = cases.matrix_scene()
    want = cases.Chain(prev, curr).frames(setting, [cases.MATRIX_FACTOR])[0]
    h, w = prev.shape[:2]
    p, c, o, e = ctx.frame_from(prev), ctx.frame_from(curr), ctx.create_frame(w, h), ctx.frame_from(want)
    r = poisoned_record(ctx)
    try:
        apply(ctx, setting)
        ctx.interpolate_frames(p, c, o, cases.MATRIX_FACTOR)
        ctx.frame_diff(o, e, r)                               # behind the interpolation on the lane: no wait in between
        summary = capi.summarize(ctx.read_diff_record(r))
        assert summary["differing"] == 0 and summary["pixels"] == w * h and summary["psnr_db"] == math.inf, summary
        ctx.frame_diff(o, p, r)                               # and the measure is not blind: the frame is not prev
        assert capi.summarize(ctx.read_diff_record(r))["differing"] > w * h // 4
    finally:
        apply(ctx, DEFAULT)
        for f in (p, c, o, e, r):
            ctx.destroy_frame(f)


# ---- 8. lfg_host --evaluate

COMPENSATED = ("--semantics", "intended", "--interpolator", "compensated")


def host_evaluate(tmp_path, frames, *options, expect_failure=False):
    """`frames` through `lfg_host --evaluate` as a raw file: the report line (or the failed process)."""
    if not os.path.exists(HOST):
        import __graft_entry__ as entry
        entry.build()
    n, (h, w) = len(frames), frames[0].shape[:2]
    tmp_path.mkdir(exist_ok=True)
    src = tmp_path / "in.rgba"
    np.concatenate([f.reshape(-1) for f in frames]).tofile(src)
    p = subprocess.run([HOST, "--input-width", str(w), "--input-height", str(h), "--frames", str(n), "--quiet", "--input-raw", str(src),
                        "--evaluate", *options], capture_output=True, text=True, timeout=300)
    if expect_failure:
        return p
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def panned(n, w=96, h=64):
    frames = [synth.make_prev(w, h, synth.BASE_SEED)]
    for _ in range(n - 1):
        frames.append(synth.translate(frames[-1], (3, -2), synth.BASE_SEED))
    return frames


def same_as_model(got, records, what):
    """A summary of the report against the model's summary of the word-wise sum of `records`."""
    total = records[0]
    for rec in records[1:]:
        total = dm.add(total, rec)
    want = dm.summarize(total, 0xF)
    assert [got[k] for k in INT_KEYS] == [want[k] for k in INT_KEYS], f"{what}: {got}, model {want}"
    assert tuple(got["sse"]) == total[1], what
    assert got["mse"] == pytest.approx(want["mse"], rel=1e-12) and abs(got["psnr_db"] - want["psnr_db"]) <= 1e-9, what


def test_host_evaluate(ctx, tmp_path):
    f = panned(5)
    report = host_evaluate(tmp_path / "compensated", f, *COMPENSATED)
    ev = report["evaluation"]
    assert report["presented"] == 0 and report["input_frames"] == 5 and ev["pairs"] == 2
    setting = ("full", -1, "compensated", 1)
    generated = [cases.Chain(f[0], f[2]).frames(setting, [0.5])[0], cases.Chain(f[2], f[4]).frames(setting, [0.5])[0]]
    same_as_model(ev["generated"], [dm.frame_diff(generated[0], f[1]), dm.frame_diff(generated[1], f[3])], "generated")
    same_as_model(ev["repeated"], [dm.frame_diff(f[0], f[1]), dm.frame_diff(f[2], f[3])], "repeated")
    assert ev["generated"]["psnr_db"] > ev["repeated"]["psnr_db"]
    # a trailing unpaired frame is ignored
    assert host_evaluate(tmp_path / "six", panned(6), *COMPENSATED)["evaluation"] == ev
    # the default route: worse than showing the previous frame again
    default = host_evaluate(tmp_path / "default", f)["evaluation"]
    shader = [cases.Chain(f[0], f[2]).frames(DEFAULT, [0.5])[0], cases.Chain(f[2], f[4]).frames(DEFAULT, [0.5])[0]]
    same_as_model(default["generated"], [dm.frame_diff(shader[0], f[1]), dm.frame_diff(shader[1], f[3])], "default route")
    assert default["repeated"] == ev["repeated"]
    assert default["generated"]["psnr_db"] < default["repeated"]["psnr_db"]


def test_host_evaluate_identical_frames(ctx, tmp_path):
    ev = host_evaluate(tmp_path, [synth.make_prev(96, 64, synth.BASE_SEED)] * 5, *COMPENSATED)["evaluation"]
    assert ev["pairs"] == 2
    for name in ("generated", "repeated"):
        assert ev[name]["differing"] == 0 and ev[name]["psnr_db"] is None and ev[name]["pixels"] == 2 * 96 * 64, ev[name]
        assert ev[name]["sse"] == [0, 0, 0, 0] and ev[name]["mse"] == 0


@pytest.mark.parametrize("options", [("--ranks", "2", "--rank", "0", "--comm-file", "unused"), ("--factors", "0.25,0.5"),
                                     ("--no-interpolation",), ("--output-raw", "unused.rgba"), ("--dump-dir", "unused"),
                                     ("--replay", "2")], ids=lambda o: o[0])
def test_host_evaluate_refuses(ctx, tmp_path, options):
    p = host_evaluate(tmp_path, panned(3, 16, 8), *options, expect_failure=True)
    assert p.returncode != 0 and p.stdout == "" and "--evaluate" in p.stderr, (p.returncode, p.stdout, p.stderr)
    assert not os.path.exists("unused.rgba") and not os.path.exists("unused")


def test_host_evaluate_needs_three_frames(ctx, tmp_path):
    p = host_evaluate(tmp_path, panned(2, 16, 8), expect_failure=True)
    assert p.returncode != 0 and p.stdout == ""
