"""Structural similarity on the GPU: lfg_frame_ssim against the CPU model (tests/ssim_model.py), every word of the record in
exact integers -- the smallest frames, every seam of the kernel's tiling, six contents, four masks, both load paths, regions of
interest, accumulation, three lanes, argument checks -- then lfg_frame_ssim_summarize, and lfg_host --evaluate's "ssim" objects
against the model over the CPU chain's frames (tests/cases.py)."""
import ctypes

import numpy as np
import pytest

from linux_fg_amd import capi
from tests import cases
from tests import diff_model as dm
from tests import ssim_model as sm
from tests.gpu_kit import DEFAULT, ctx, pitched, three_lanes
from tests.test_gpu_diff import COMPENSATED, host_evaluate, panned

pytestmark = pytest.mark.gpu

RECORD_TEXELS = ctypes.sizeof(capi.FrameSsimStats) // 4
SW, SR, GW, GPC = capi.SSIM_STRIP_WINDOWS, capi.SSIM_SEGMENT_ROWS, capi.SSIM_GROUP_WAVES, capi.SSIM_GROUPS_PER_CU
MI355X_CUS = 256                                              # what the second grid-stride trip below is sized for


def size(windows_x, windows_y, rest_x=0, rest_y=0):
    """The frame of windows_x by windows_y windows with rest_x, rest_y < 4 columns and rows that are not looked at."""
    return 4 * (windows_x + 1) + rest_x, 4 * (windows_y + 1) + rest_y


SMALLEST = [(8, 8), (9, 8), (12, 8), (8, 12), (11, 11)]
SEAM_SIZES = [
    size(SW - 1, SR - 1), size(SW, SR), size(SW + 1, SR + 1),               # a wave's 62nd, 63rd and 64th window; an item's 7th .. 9th row
    size(SW, SR, 3, 3), size(2 * SW, 2 * SR), size(2 * SW + 1, 2 * SR + 1, 3, 1),
    size(1, GW * SR), size(1, GW * SR + 1, 1, 2),                           # a workgroup's 4 items, and the first item of a second one
    size(SW + 1, 2 * SR + 1, 2, 0),                                         # 2 strips by 3 segments: 6 items in two workgroups
]


def poisoned_record(ctx):
    r = ctx.create_ssim_record()
    ctx.upload(r, np.full((1, RECORD_TEXELS, 4), 0xFF, np.uint8))
    return r


def describe(got, want):
    bins = [(k, g, e) for k, (g, e) in enumerate(zip(got[2], want[2])) if g != e]
    return (f"windows {got[0]} / {want[0]}, sum {got[1]} / {want[1]}, worst {got[3]:#x} / {want[3]:#x}, {len(bins)} bins differ, "
            f"first (bin, got, model) {bins[:4]}")


def check_against_the_model(ctx, a, b, fa, fb, what, masks=sm.MASKS):
    """lfg_frame_ssim(fa, fb) under every mask, twice into one poisoned record: both results are the model's of (a, b)."""
    q = sm.quotients(a, b)
    r = poisoned_record(ctx)
    try:
        for mask in masks:
            want = sm.record(q, mask)
            ctx.frame_ssim(fa, fb, r, mask)
            first = ctx.read_ssim_record(r)
            ctx.frame_ssim(fa, fb, r, mask)                   # into the same record: it writes, it does not accumulate
            again = ctx.read_ssim_record(r)
            assert first == want, f"{what} mask {mask:#x}: {describe(first, want)}"
            assert again == want, f"{what} mask {mask:#x}, second call: {describe(again, want)}"
    finally:
        ctx.destroy_frame(r)


def check_pair(ctx, a, b, what, masks=sm.MASKS):
    fa, fb = ctx.frame_from(a), ctx.frame_from(b)
    try:
        check_against_the_model(ctx, a, b, fa, fb, what, masks)
    finally:
        ctx.destroy_frame(fa)
        ctx.destroy_frame(fb)


# ---- 1. equals the model exactly: the smallest frames, the wave's 63 windows, an item's 8 rows, the workgroup's 4 items

@pytest.mark.parametrize("w,h", SMALLEST + SEAM_SIZES)
def test_equals_the_model(ctx, w, h):
    for name, (a, b) in sm.scenes(w, h).items():
        check_pair(ctx, a, b, f"{name} {w}x{h}", masks=sm.MASKS if name == "graded" else (0xF, 0x5))


def test_1080p(ctx):
    a, b = dm.graded_of(1920, 1080)
    check_pair(ctx, a, b, "graded 1920x1080")


def test_second_grid_stride_trip(ctx):
    """One window wide and one segment more than a grid of MI355X_CUS CUs has waves: the first wave walks twice."""
    w, h = size(1, SR * MI355X_CUS * GPC * GW + 1)
    a, b = dm.graded_of(w, h)

    def tall(host):
        """`host`, taller than lfg_frame_create makes a frame, as a view of its bytes in the rows of a 2048-wide one."""
        rows = -(-host.size // (2048 * 4))
        flat = np.zeros(rows * 2048 * 4, np.uint8)
        flat[:host.size] = host.reshape(-1)
        big = ctx.frame_from(flat.reshape(rows, 2048, 4))
        return big, capi.Context.wrap(big.data, w, h, pitch=w * 4)

    (big_a, fa), (big_b, fb) = tall(a), tall(b)
    try:
        check_against_the_model(ctx, a, b, fa, fb, f"graded {w}x{h}", masks=(0xF,))
    finally:
        ctx.destroy_frame(big_a)
        ctx.destroy_frame(big_b)


# ---- 2. both load paths

def pads_to_16(w):
    """Two different pads that make both row pitches multiples of 16, so that the 16-byte path runs at any width."""
    first = (-w) % 4 or 4
    return first, first + 4


PITCHED_SIZES = [(11, 11), size(SW, SR, 1, 0), size(SW + 1, SR + 1, 3, 2)]


@pytest.mark.parametrize("pads", [(3, 5), (4, 8), (2, 6), "16"], ids=lambda p: f"pads-{p}")
@pytest.mark.parametrize("w,h", PITCHED_SIZES)
def test_pitched(ctx, w, h, pads):
    """Pads that leave the pitch at 4, 8 or 0 modulo 16 whatever the width: (3, 5) and (4, 8) make the two frames' pitches
    differ modulo 16, (2, 6) makes them agree, "16" makes both multiples of 16 -- the one case of the 16-byte loads."""
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


def test_pitches_cover_both_paths_and_every_residue():
    residues = set()
    for w, _ in PITCHED_SIZES:
        for pads in [(3, 5), (4, 8), (2, 6), pads_to_16(w)]:
            residues |= {(w + p) * 4 % 16 for p in pads}
    assert residues >= {0, 4, 8}


@pytest.mark.parametrize("w,h", [(8, 8), size(SW + 1, 3, 1, 1)])
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


def test_region_of_interest_and_the_same_frame(ctx):
    (a, b), (w, h, x, y) = dm.graded_of(400, 120), (4 * (SW + 2) + 1, 41, 7, 3)
    fa, fb = ctx.frame_from(a), ctx.frame_from(b)
    try:
        for x0 in (x, 8):                                     # 8: a window whose base and pitch are multiples of 16
            va = capi.Context.wrap(fa.data + (y * 400 + x0) * 4, w, h, pitch=fa.pitch)
            vb = capi.Context.wrap(fb.data + (y * 400 + x0) * 4, w, h, pitch=fb.pitch)
            check_against_the_model(ctx, a[y:y + h, x0:x0 + w], b[y:y + h, x0:x0 + w], va, vb, f"window at ({x0}, {y})")
        check_against_the_model(ctx, a, a, fa, fa, "the same frame twice", masks=(0xF, 0x8))
        upper, lower = capi.Context.wrap(fa.data, 400, 119), capi.Context.wrap(fa.data + 1600, 400, 119)
        check_against_the_model(ctx, a[:-1], a[1:], upper, lower, "overlapping views", masks=(0x7,))
        assert (ctx.download(fa) == a).all() and (ctx.download(fb) == b).all()
    finally:
        ctx.destroy_frame(fa)
        ctx.destroy_frame(fb)


# ---- 3. accumulate

def test_accumulate(ctx):
    sizes = [(200, 120), size(SW + 1, 2, 1, 3), (8, 8)]
    pairs = [dm.graded(w, h, 50 + k) for k, (w, h) in enumerate(sizes)]
    pairs[2] = sm.checkerboard(8, 8)                          # the lowest value there is: `worst` must come from the last pair
    frames = [(ctx.frame_from(a), ctx.frame_from(b)) for a, b in pairs]
    quotients = [sm.quotients(a, b) for a, b in pairs]
    r = poisoned_record(ctx)
    try:
        for mask in (0xF, 0x5):
            models = [sm.record(q, mask) for q in quotients]
            for k, (fa, fb) in enumerate(frames):             # no host wait between them
                ctx.frame_ssim(fa, fb, r, mask, accumulate=k > 0)
            got = ctx.read_ssim_record(r)
            want = sm.add(sm.add(models[0], models[1]), models[2])
            assert got == want, describe(got, want)
            assert got[0] == sum((w // 4 - 1) * (h // 4 - 1) for w, h in sizes) and got[3] == models[2][3]
            ctx.frame_ssim(*frames[1], r, mask)               # accumulate 0 on a record that holds something
            assert ctx.read_ssim_record(r) == models[1]
            ctx.frame_ssim(*frames[1], r, mask, accumulate=True)
            assert ctx.read_ssim_record(r) == sm.add(models[1], models[1])
            ctx.frame_ssim(*frames[0], r, mask, accumulate=True)      # a higher `worst` leaves the lower one
            assert ctx.read_ssim_record(r) == sm.add(sm.add(models[1], models[1]), models[0])
    finally:
        for f in [r] + [f for pair in frames for f in pair]:
            ctx.destroy_frame(f)


# ---- 4. three lanes

LANE_SIZES = [(200, 120), (64, 36), (33, 17), (8, 8), (130, 90), size(SW + 1, 1), (257, 131), (11, 9), size(1, GW * SR + 1)]


def test_three_lanes(ctx):
    inputs = [dm.graded(w, h, 80 + k) for k, (w, h) in enumerate(LANE_SIZES)]
    masks = [sm.MASKS[k % len(sm.MASKS)] for k in range(len(inputs))]

    def enqueue(i, a, b):
        fa, fb, r = ctx.frame_from(a), ctx.frame_from(b), poisoned_record(ctx)
        ctx.frame_ssim(fa, fb, r, masks[i])
        return fa, fb, r

    alone = []
    for i, (a, b) in enumerate(inputs):
        fs = enqueue(i, a, b)
        alone.append(ctx.download(fs[-1]))
        assert ctx.read_ssim_record(fs[-1]) == sm.frame_ssim(a, b, masks[i])
        for f in fs:
            ctx.destroy_frame(f)
    three_lanes(ctx, inputs, enqueue, alone)


# ---- 5. validation launches nothing

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
    narrow, flat = capi.Context.wrap(fa.data, 7, h, pitch=fa.pitch), capi.Context.wrap(fa.data, w, 7, pitch=fa.pitch)
    # (described only: refused before anything reads them) one block column or row more than `worst`'s 16-bit fields hold
    broad, tall = capi.Context.wrap(fa.data, 262148, 8), capi.Context.wrap(fa.data, 8, 262148)
    empty = capi.Frame()
    r = poisoned_record(ctx)
    rec = ctypes.c_void_p(r.data)

    def ssim(x, y, mask=0xF, accumulate=0, stats=rec):
        return lib.lfg_frame_ssim(ctx.h, x and B(x), y and B(y), mask, accumulate, stats)

    bad = [
        ssim(None, fb), ssim(fa, None), ssim(empty, fb), ssim(fa, empty), ssim(fa, fb, stats=None),      # NULL pointers, no frame
        ssim(fa, fb, stats=ctypes.c_void_p(r.data + 4)),                                                 # not 8-byte aligned
        ssim(mv, fb), ssim(fa, mv), ssim(mv, mv),                                                        # wrong format
        ssim(small, fb), ssim(fa, small), ssim(fa, short), ssim(short, fb),                              # differing sizes
        ssim(odd, fb), ssim(fa, odd), ssim(shifted, fb), ssim(fa, shifted),                              # pitch, alignment
        ssim(fa, fb, 0), ssim(fa, fb, 16), ssim(fa, fb, 0xFFFFFFFF),                                     # the mask
        ssim(fa, fb, accumulate=2), ssim(fa, fb, accumulate=-1),                                         # accumulate
        ssim(narrow, narrow), ssim(flat, flat),                                                          # W < 8, H < 8
        ssim(broad, broad), ssim(tall, tall),                                                            # W, H > 262,144
    ]
    assert all(rc == -1 for rc in bad), bad                   # LFG_ERR_INVALID
    assert lib.lfg_last_error(ctx.h).decode()
    assert lib.lfg_frame_ssim(None, B(fa), B(fb), 0xF, 0, rec) == -1
    ctx.sync()
    assert (ctx.download(r) == 0xFF).all()                    # the record keeps its poison
    assert (ctx.download(fa) == a).all() and (ctx.download(fb) == b).all()
    # the valid call next to the bad ones works, and writes nothing but the record
    ctx.frame_ssim(fa, fb, r)
    assert ctx.read_ssim_record(r) == sm.frame_ssim(a, b, 0xF)
    assert (ctx.download(fa) == a).all() and (ctx.download(fb) == b).all()
    for f in (fa, fb, mv, small, short, wide, r):
        ctx.destroy_frame(f)


# ---- 6. lfg_frame_ssim_summarize on what the device wrote

def test_summarize(ctx):
    lib = ctx.lib
    for name, (a, b) in sm.scenes(96, 64).items():
        fa, fb, r = ctx.frame_from(a), ctx.frame_from(b), poisoned_record(ctx)
        try:
            ctx.frame_ssim(fa, fb, r, 0x7)
            rec = ctx.read_ssim_record(r)
            assert capi.summarize_ssim(rec, 0x7) == sm.summarize(sm.frame_ssim(a, b, 0x7), 0x7), name
        finally:
            for f in (fa, fb, r):
                ctx.destroy_frame(f)
    s = capi.FrameSsimStats(rec[0], (ctypes.c_int64 * 4)(*rec[1]), (ctypes.c_uint64 * 65)(*rec[2]), rec[3])
    out = capi.FrameSsimSummary()
    assert lib.lfg_frame_ssim_summarize(ctypes.byref(s), 0x7, ctypes.byref(out)) == 0
    s.hist[3] += 1                                            # a histogram that does not sum to windows
    assert lib.lfg_frame_ssim_summarize(ctypes.byref(s), 0x7, ctypes.byref(out)) == -1
    s.hist[3] -= 1
    s.windows = 0                                             # no windows
    assert lib.lfg_frame_ssim_summarize(ctypes.byref(s), 0x7, ctypes.byref(out)) == -1


# ---- 7. lfg_host --evaluate

SSIM_KEYS = ["windows", "all", "db", "channels", "sum", "identical", "below_half", "worst"]
OLD_KEYS = ["pixels", "differing", "over_1", "max_abs", "p50", "p99", "mse", "psnr_db", "sse"]


def same_as_model(got, pairs, what):
    """An "ssim" object of the report against the model's summary of the accumulated records of `pairs`."""
    total = None
    for a, b in pairs:
        rec = sm.frame_ssim(a, b, 0xF)
        total = rec if total is None else sm.add(total, rec)
    want = sm.summarize(total, 0xF)
    assert list(got) == SSIM_KEYS and list(got["worst"]) == ["value", "x", "y"], what
    assert (got["windows"], tuple(got["sum"]), got["identical"], got["below_half"], got["worst"]["x"], got["worst"]["y"]) == \
           (want["windows"], total[1], want["identical"], want["below_half"], want["worst_x"], want["worst_y"]), f"{what}: {got}, model {want}"
    doubles = [(got["all"], want["all"]), (got["db"], want["db"]), (got["worst"]["value"], want["worst_value"])] + \
        list(zip(got["channels"], want["ssim"]))
    for g, e in doubles:
        assert abs(g - e) <= 1e-12, f"{what}: {got}, model {want}"


def test_host_evaluate(ctx, tmp_path):
    f = panned(5)
    ev = host_evaluate(tmp_path / "compensated", f, *COMPENSATED)["evaluation"]
    setting = ("full", -1, "compensated", 1)
    generated = [cases.Chain(f[0], f[2]).frames(setting, [0.5])[0], cases.Chain(f[2], f[4]).frames(setting, [0.5])[0]]
    same_as_model(ev["generated"]["ssim"], [(generated[0], f[1]), (generated[1], f[3])], "generated")
    same_as_model(ev["repeated"]["ssim"], [(f[0], f[1]), (f[2], f[3])], "repeated")
    assert ev["generated"]["ssim"]["windows"] == 2 * 345
    default = host_evaluate(tmp_path / "default", f)["evaluation"]
    shader = [cases.Chain(f[0], f[2]).frames(DEFAULT, [0.5])[0], cases.Chain(f[2], f[4]).frames(DEFAULT, [0.5])[0]]
    same_as_model(default["generated"]["ssim"], [(shader[0], f[1]), (shader[1], f[3])], "default route")
    assert default["repeated"] == ev["repeated"]
    # every key that was there before is where it was, with "ssim" behind it; its values are tests/test_gpu_diff.py's to hold
    for report in (ev, default):
        assert list(report) == ["pairs", "generated", "repeated"]
        for name in ("generated", "repeated"):
            assert list(report[name]) == OLD_KEYS + ["ssim"]
    total = dm.add(dm.frame_diff(generated[0], f[1]), dm.frame_diff(generated[1], f[3]))
    want = dm.summarize(total, 0xF)
    assert [ev["generated"][k] for k in OLD_KEYS[:6]] == [want[k] for k in OLD_KEYS[:6]] and tuple(ev["generated"]["sse"]) == total[1]


def test_host_evaluate_identical_frames(ctx, tmp_path):
    from linux_fg_amd import synth
    ev = host_evaluate(tmp_path, [synth.make_prev(96, 64, synth.BASE_SEED)] * 5, *COMPENSATED)["evaluation"]
    for name in ("generated", "repeated"):
        s = ev[name]["ssim"]
        assert s["all"] == 1.0 and s["db"] is None and s["identical"] == s["windows"] == 690 and s["below_half"] == 0, s
        assert s["channels"] == [1.0] * 4 and s["sum"] == [690 << 24] * 4 and s["worst"] == {"value": 1.0, "x": 0, "y": 0}


def test_host_evaluate_below_one_window(ctx, tmp_path):
    rng = np.random.default_rng(4)
    ev = host_evaluate(tmp_path, [rng.integers(0, 256, (4, 4, 4), dtype=np.uint8) for _ in range(3)])["evaluation"]
    assert ev["pairs"] == 1
    for name in ("generated", "repeated"):
        assert list(ev[name]) == OLD_KEYS + ["ssim"] and ev[name]["ssim"] is None and ev[name]["pixels"] == 16
