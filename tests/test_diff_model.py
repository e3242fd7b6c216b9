"""lfg_frame_diff_summarize (a pure host function: no GPU) against the CPU model (tests/diff_model.py), the quantile rule at its
edges on hand-made records, the power of the graded inputs that the GPU tests take, and the quality table of DESIGN.md section
4.11 on the CPU chain.  CPU only."""
import ctypes
import math
import os

import numpy as np
import pytest

from linux_fg_amd import synth
from tests import cases
from tests import diff_model as dm

# the sizes of tests/test_gpu_diff.py (imported there)
SEAM_SIZES = [(1, 1), (3, 2), (4, 1), (5, 3), (63, 5), (64, 4), (65, 9), (255, 2), (256, 2), (257, 131), (1023, 2), (1024, 2),
              (1025, 3), (200, 120)]
INT_KEYS = ("pixels", "differing", "over_1", "max_abs", "p50", "p99")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as entry
    from linux_fg_amd import capi as c
    if not os.path.exists(c.LIB_PATH):
        entry.build()
    return c



def same_summary(got, want, what=""):
    assert [got[k] for k in INT_KEYS] == [want[k] for k in INT_KEYS], f"{what}: {got} against the model's {want}"
    assert got["mse"] == pytest.approx(want["mse"], rel=1e-12, abs=0.0), what
    if math.isinf(want["psnr_db"]):
        assert got["psnr_db"] == math.inf, what                       # HUGE_VAL
    else:
        assert got["psnr_db"] == pytest.approx(want["psnr_db"], rel=1e-12, abs=0.0), what


def record(pixels, **bins):
    """A hand-made record: hist from b<k>=count keywords, sse all zero."""
    hist = [0] * 256
    for name, count in bins.items():
        hist[int(name[1:])] = count
    return pixels, (0, 0, 0, 0), tuple(hist)


# ---- the function against the model

@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 4), (200, 120)])
def test_summarize_equals_the_model(capi, w, h):
    a, b = dm.graded_of(w, h)
    for mask in dm.MASKS:
        rec = dm.frame_diff(a, b, mask)
        same_summary(capi.summarize(rec, mask), dm.summarize(rec, mask), f"{w}x{h} mask {mask:#x}")
    # several pairs in one record, as accumulate = 1 leaves it
    both = dm.add(dm.frame_diff(a, b, 0x7), dm.frame_diff(b, b, 0x7))
    same_summary(capi.summarize(both, 0x7), dm.summarize(both, 0x7), "accumulated")
    assert capi.summarize(both, 0x7)["pixels"] == 2 * w * h


def test_identical_frames_give_huge_val(capi):
    a = cases.textured(33, 7, 5)
    rec = dm.frame_diff(a, a, 0xF)
    assert rec == (231, (0, 0, 0, 0), (231,) + (0,) * 255)
    got = capi.summarize(rec, 0xF)
    assert got["psnr_db"] == math.inf and got["mse"] == 0.0
    assert [got[k] for k in INT_KEYS] == [231, 0, 0, 0, 0, 0]
    same_summary(got, dm.summarize(rec, 0xF))


def test_mse_takes_the_channels_of_the_mask(capi):
    rec = (10, (10, 200, 3000, 40000), (0,) * 255 + (10,))
    for mask, total in [(0x1, 10), (0x2, 200), (0x8, 40000), (0x5, 3010), (0xA, 40200), (0x7, 3210), (0xF, 43210)]:
        got = capi.summarize(rec, mask)
        assert got["mse"] == pytest.approx(total / (bin(mask).count("1") * 10), rel=1e-12)
        assert got["psnr_db"] == pytest.approx(10 * math.log10(65025 / got["mse"]), rel=1e-12)
        same_summary(got, dm.summarize(rec, mask), f"mask {mask:#x}")
    worst = capi.summarize((1, (65025,) * 4, (0,) * 255 + (1,)), 0xF)
    assert worst["mse"] == 65025.0 and worst["psnr_db"] == 0.0 and worst["max_abs"] == 255


def test_every_error_return(capi):
    lib = capi.load()
    good = dm.frame_diff(*dm.graded_of(5, 3), 0xF)

    def call(rec, mask, out=True, stats=True):
        s = capi.FrameDiffStats(rec[0], (ctypes.c_uint64 * 4)(*rec[1]), (ctypes.c_uint64 * 256)(*rec[2]))
        return lib.lfg_frame_diff_summarize(ctypes.byref(s) if stats else None, mask, ctypes.byref(capi.FrameDiffSummary()) if out else None)

    assert call(good, 0xF) == 0 and call(good, 1) == 0
    assert call(good, 0xF, stats=False) == -1 and call(good, 0xF, out=False) == -1                 # a NULL pointer
    assert call(good, 0) == -1 and call(good, 16) == -1 and call(good, 0xFFFFFFFF) == -1           # the mask
    assert call((0, (0,) * 4, (0,) * 256), 0xF) == -1                                              # no pixels
    pixels, sse, hist = good
    assert call((pixels + 1, sse, hist), 0xF) == -1 and call((pixels - 1, sse, hist), 0xF) == -1   # hist does not sum to pixels
    assert call((pixels, sse, (hist[0] + 1,) + hist[1:]), 0xF) == -1
    assert call((1, (0,) * 4, (2 ** 63, 2 ** 63 + 1) + (0,) * 254), 0xF) == -1                     # ... not even modulo 2^64
    assert call((2 ** 64 - 1, (0,) * 4, (0xFF,) * 256), 0xF) == -1                                 # a poisoned record's shape
    for bad in [(good, 0), (good, 16), ((0, (0,) * 4, (0,) * 256), 0xF), ((pixels + 1, sse, hist), 0xF)]:
        assert dm.summarize(*bad) is None
        with pytest.raises(capi.LfgError):
            capi.summarize(*bad)


# ---- the quantile rule at its edges: the smallest k with 100 * (hist[0] + .. + hist[k]) >= P * pixels

@pytest.mark.parametrize("zeros,p50", [(99, 1), (100, 0), (101, 0)])
def test_p50_at_its_edge(capi, zeros, p50):
    rec = record(200, b0=zeros, b1=200 - zeros)                       # 100 * 100 = 50 * 200
    got = capi.summarize(rec)
    assert got["p50"] == p50 and got["p99"] == 1 and got["differing"] == 200 - zeros and got["over_1"] == 0
    same_summary(got, dm.summarize(rec))


@pytest.mark.parametrize("low,p99", [(197, 7), (198, 3), (199, 3)])
def test_p99_at_its_edge(capi, low, p99):
    rec = record(200, b0=150, b3=low - 150, b7=200 - low)             # 100 * 198 = 99 * 200
    got = capi.summarize(rec)
    assert got["p99"] == p99 and got["p50"] == 0 and got["max_abs"] == 7 and got["over_1"] == 50
    same_summary(got, dm.summarize(rec))


def test_quantiles_skip_empty_bins_and_large_counts(capi):
    rec = record(3, b0=1, b9=1, b255=1)                               # 100 >= 150? no; 200 >= 150: p50 = 9; p99 = 255
    assert (capi.summarize(rec)["p50"], capi.summarize(rec)["p99"]) == (9, 255)
    big = 2 ** 56                                                     # 100 * below no longer fits 63 bits
    rec = record(2 * big, b2=big, b5=big)
    got = capi.summarize(rec)
    assert (got["p50"], got["p99"], got["differing"], got["over_1"]) == (2, 5, 2 * big, 2 * big)
    same_summary(got, dm.summarize(rec))


# ---- the graded inputs of the GPU tests are informative

@pytest.mark.parametrize("w,h", [s for s in SEAM_SIZES if s[0] * s[1] >= 256])
def test_graded_inputs_are_informative(w, h):
    a, b = dm.graded_of(w, h)
    hists = {mask: dm.frame_diff(a, b, mask)[2] for mask in (0xF, 0x7, 0x8)}
    full = hists[0xF]
    assert full[0] > 0 and full[1] > 0 and full[255] >= 2, (full[0], full[1], full[255])
    assert sum(1 for v in full if v > 0) >= 30
    assert hists[0xF] != hists[0x7] and hists[0xF] != hists[0x8] and hists[0x7] != hists[0x8]
    for mask, hist in hists.items():
        assert sum(hist) == w * h, mask
    sse = dm.frame_diff(a, b, 0xF)[1]
    assert len(set(sse)) == 4                                         # a swap of two channels' sums would show


# ---- the quality table on the CPU chain

def test_quality_table_on_the_cpu_chain(capi):
    """96 x 64, a pan of (3, -2) per frame, the pair is frames 0 and 2 and frame 1 is held out; PSNR over R, G and B."""
    w, h = 96, 64
    f0 = synth.make_prev(w, h, synth.BASE_SEED)
    f1 = synth.translate(f0, (3, -2), synth.BASE_SEED)
    f2 = synth.translate(f1, (3, -2), synth.BASE_SEED)
    chain = cases.Chain(f0, f2)

    def measured(frame):
        return capi.summarize(dm.frame_diff(frame, f1, 0x7), 0x7)

    repeat = measured(f0)
    shader = measured(chain.frames(("full", -1, "shader", 0), [0.5])[0])
    pyramid = measured(chain.frames(("pyramid", -1, "compensated", 1), [0.5])[0])
    full = measured(chain.frames(("full", -1, "compensated", 1), [0.5])[0])
    print({k: (round(v["psnr_db"], 2), v["differing"]) for k, v in
           {"repeat": repeat, "shader/reference": shader, "pyramid+compensated": pyramid, "full+compensated": full}.items()})
    assert shader["psnr_db"] < repeat["psnr_db"] < pyramid["psnr_db"] < full["psnr_db"]
    assert full["differing"] == 9 and full["pixels"] == 6144
