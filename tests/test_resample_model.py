"""lfg_resample where it needs no GPU: the library's one table builder (lfg_resample_taps) against the float64 model of the
definition (tests/resample_model.py), and what the definition promises, shown on the model -- whose bytes the GPU is held to:
identity, the distance from the float64 evaluation, anti-aliasing where lfg_scale point-samples.  CPU only."""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import scale_f64 as f64
from tests import resample_model as rm
from tests import sharpen_model as sm

INT_BOUND = 0.75                 # LSB against the float64 evaluation: the output is one of the two integers next to it
STRIPE_LEVELS = 64               # the 0 / 255 stripes at 3 : 1 span at most this many levels under every filter but nearest


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as entry
    from linux_fg_amd import capi as c
    if not os.path.exists(c.LIB_PATH):
        entry.build()
    return c


@functools.lru_cache(maxsize=None)
def table(filt, n_in, n_out):
    return rm.table(filt, n_in, n_out)


@pytest.mark.parametrize("filt", rm.FILTERS, ids=[rm.NAMES[f] for f in rm.FILTERS])
def test_the_librarys_table_is_the_models(capi, filt):
    assert getattr(capi, "FILTER_" + rm.NAMES[filt].upper().replace("-", "_")) == filt
    for n_in, n_out in rm.RATIOS:
        first, count, weights = capi.resample_taps(filt, n_in, n_out)
        want_first, want_count, want_q, _ = table(filt, n_in, n_out)
        what = f"{rm.NAMES[filt]} {n_in}->{n_out}"
        assert (first == want_first).all() and (count == want_count).all(), what
        assert np.abs(weights.astype(np.int32) - want_q.astype(np.int32)).max() <= 1, what
        assert (weights.astype(np.int32).sum(axis=1) == rm.ONE).all(), what
        assert np.abs(weights.astype(np.int32)).sum(axis=1).max() <= 32768, what
        live = np.arange(rm.MAX_TAPS)[None, :] < count[:, None]
        assert (weights[~live] == 0).all(), what
        assert (first >= 0).all() and (first + count.astype(np.int64) <= n_in).all(), what


def test_nearest_is_one_tap_at_the_stated_index(capi):
    for n_in, n_out in rm.RATIOS:
        first, count, weights = capi.resample_taps(capi.FILTER_NEAREST, n_in, n_out)
        p = np.arange(n_out)
        assert (first == (2 * p + 1) * n_in // (2 * n_out)).all() and (count == 1).all()
        assert (weights[:, 0] == rm.ONE).all() and (weights[:, 1:] == 0).all()


def test_identity(capi):
    """in == out: every filter but Mitchell, which is no interpolating kernel, returns the input bytes."""
    frame = sm.noise(24, 16, 3)
    for filt in rm.FILTERS:
        tx, ty = capi.resample_taps(filt, 24, 24), capi.resample_taps(filt, 16, 16)
        same = (rm.resample_int(frame, tx, ty) == frame).all()
        assert same == (filt != rm.MITCHELL), rm.NAMES[filt]


def test_integer_pipeline_against_float64():
    """|out - clip(V)| < 0.75 LSB, V the float64 separable evaluation with the unquantised weights: measured 0.52."""
    worst = 0.0
    widths, heights = [r for r in rm.RATIOS], [(9, 20), (7, 10), (8, 16), (7, 9), (16, 16), (19, 6), (40, 5), (56, 6), (42, 4)]
    for filt in rm.FILTERS:
        for (w, ow), (h, oh) in zip(widths, heights):
            tx, ty = table(filt, w, ow), table(filt, h, oh)
            for frame in (sm.noise(w, h, 10 * w + h), rm.binary_noise(w, h, 20 * w + h)):
                d = np.abs(rm.resample_int(frame, tx, ty).astype(np.float64) - np.clip(rm.resample_f64(frame, tx, ty), 0.0, 255.0)).max()
                worst = max(worst, d)
                assert d < INT_BOUND, (rm.NAMES[filt], w, h, ow, oh, d)
    print(f"integer pipeline against float64: {worst:.4f} LSB at the most")


@pytest.mark.parametrize("transposed", [False, True], ids=["columns", "rows"])
def test_stripes_are_averaged_not_sampled(capi, transposed):
    """96 x 4 one-pixel stripes to 32 x 4: the reference's six taps give 0, 255, 0, 255, ... again (the float64 model of
    lfg_scale); every filter here but nearest gives a flat grey."""
    frame = rm.stripes(96, 4)
    frame = np.ascontiguousarray(frame.transpose(1, 0, 2)) if transposed else frame
    ow, oh = (4, 32) if transposed else (32, 4)
    h, w = frame.shape[:2]
    reference = np.rint(np.clip(f64.scale_f64(frame, ow, oh), 0.0, 255.0))
    assert reference.min() == 0 and reference.max() == 255
    for filt in rm.FILTERS:
        out = rm.resample_int(frame, capi.resample_taps(filt, w, ow), capi.resample_taps(filt, h, oh)).astype(np.int32)
        levels = int(out.max() - out.min())
        print(f"{rm.NAMES[filt]}: {out.min()} .. {out.max()}")
        if filt == rm.NEAREST:
            assert levels == 255
        else:
            assert levels <= STRIPE_LEVELS and 96 <= out.min() and out.max() <= 160, (rm.NAMES[filt], out.min(), out.max())


def test_the_tap_limit(capi):
    """out = 9: the largest `in` whose rows have at most 64 taps (from the model's integer tap rule) is accepted, in + 1 is
    LFG_ERR_UNSUPPORTED.  Nearest has one tap at every ratio."""
    for filt in rm.FILTERS:
        if filt == rm.NEAREST:
            capi.resample_taps(filt, 100000, 9)
            continue
        largest = max(n for n in range(9, 400) if rm.max_taps(filt, n, 9) <= rm.MAX_TAPS)
        assert rm.max_taps(filt, largest + 1, 9) > rm.MAX_TAPS
        first, count, weights = capi.resample_taps(filt, largest, 9)
        assert count.max() <= rm.MAX_TAPS and (weights.astype(np.int32).sum(axis=1) == rm.ONE).all()
        with pytest.raises(capi.LfgError) as e:
            capi.resample_taps(filt, largest + 1, 9)
        assert e.value.code == capi.ERR_UNSUPPORTED, rm.NAMES[filt]
    assert max(n for n in range(9, 400) if rm.max_taps(rm.LANCZOS3, n, 9) <= rm.MAX_TAPS) == 96       # 10.67 : 1


def test_invalid_arguments(capi):
    lib = capi.load()
    first, count = (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 4)()
    weights = (ctypes.c_int16 * (4 * capi.RESAMPLE_MAX_TAPS))()
    assert lib.lfg_resample_taps(capi.FILTER_BILINEAR, 8, 4, first, count, weights) == 0
    bad = [(capi.FILTER_BILINEAR, 0, 4, first, count, weights), (capi.FILTER_BILINEAR, 8, 0, first, count, weights),
           (capi.FILTER_BILINEAR, 8, 4, None, count, weights), (capi.FILTER_BILINEAR, 8, 4, first, None, weights),
           (capi.FILTER_BILINEAR, 8, 4, first, count, None), (-1, 8, 4, first, count, weights), (6, 8, 4, first, count, weights)]
    assert [lib.lfg_resample_taps(*b) for b in bad] == [capi.ERR_INVALID] * len(bad)
    assert lib.lfg_resample(None, None, None, capi.FILTER_BILINEAR) == capi.ERR_INVALID


def test_the_plan_of_the_benchmark_sizes():
    """What the kernel's tile plan gives for the sizes tools/resample_bench.py times."""
    plans = {(a, b): rm.plan_rows(*table(rm.LANCZOS3, a, b)[:2]) for a, b in ((1080, 2160), (1080, 1440), (2160, 1080), (2160, 720))}
    assert plans == {(1080, 2160): (16, 14), (1080, 1440): (16, 18), (2160, 1080): (16, 42), (2160, 720): (16, 62)}
