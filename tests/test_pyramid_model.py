"""The CPU model of lfg_motion_pyramid (tests/pyramid_model.py) against known answers, and the library's new exports.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from linux_fg_amd import synth
from tests import cases
from tests import pyramid_model as pm


def test_level_sizes_and_rounding_on_odd_sizes():
    assert pm.level_sizes(5, 3, 2) == [(5, 3), (3, 2), (2, 1)]
    assert pm.level_sizes(1, 1, 4) == [(1, 1)] * 5
    assert pm.level_sizes(3840, 2160, 2) == [(3840, 2160), (1920, 1080), (960, 540)]
    img = np.zeros((3, 5, 4), np.uint8)
    img[..., 0] = np.array([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10], [11, 12, 13, 14, 15]])
    img[..., 3] = 255
    r = pm.reduce(img)
    assert r.shape == (2, 3, 4)
    # (sum + 2) >> 2, the last column and row clamped
    assert r[0, 0, 0] == (1 + 2 + 6 + 7 + 2) >> 2
    assert r[0, 2, 0] == (5 + 5 + 10 + 10 + 2) >> 2
    assert r[1, 0, 0] == (11 + 12 + 11 + 12 + 2) >> 2
    assert r[1, 2, 0] == (15 * 4 + 2) >> 2
    assert (r[..., 3] == 255).all() and (r[..., 1] == 0).all()
    r2 = pm.reduce(r)
    assert r2.shape == (1, 2, 4)


def test_identical_frames_give_zero():
    prev = synth.make_prev(48, 40)
    mv = pm.motion_pyramid(prev, prev, 2, 8, 2)
    assert (mv == 0).all()


def test_flat_frames_give_zero():
    flat = np.full((24, 40, 4), 77, np.uint8)
    assert (pm.motion_pyramid(flat, flat, 1, 6, 1) == 0).all()
    assert (pm.motion_pyramid(flat, flat.copy(), 3, 5, 2) == 0).all()


@pytest.mark.parametrize("axis", [0, 1])
def test_tie_between_equal_length_vectors(axis):
    """curr repeats every 4 px along one axis and prev is curr moved by 2 along it: v and -v match exactly.  Of the two the
    smaller vy (vertical) or, vy equal, the smaller vx (horizontal) wins."""
    prev, curr, params, want = cases.pyramid_tie(axis)
    assert params == (1, 4, 2) and want == ((-2, 0) if axis == 0 else (0, -2))
    mv = pm.motion_pyramid(prev, curr, *params)
    inner = mv[12:-12, 12:-12].reshape(-1, 2)
    assert (inner == np.array(want, np.int8)).all(), np.unique(inner, axis=0)


def test_translated_noise_40_minus_24():
    W, H = 256, 192
    prev = synth.make_prev(W, H)
    curr = synth.translate(prev, (40, -24))
    mv = pm.motion_pyramid(prev, curr, 2, 16, 2)
    # the translated region is x >= 40, y < H - 24; 64 px inside it
    inner = mv[64:H - 24 - 64, 40 + 64:W - 64].reshape(-1, 2)
    assert inner.size and (inner == np.array([-40, 24], np.int8)).all()


def test_roi_form_equals_whole_frame():
    prev, curr = synth.make_pair(96, 64, shift=(9, -5))
    for params in ((1, 12, 1), (2, 16, 2), (3, 6, 3)):
        whole = pm.motion_pyramid(prev, curr, *params)
        for roi in ((0, 0, 96, 64), (5, 3, 17, 11), (80, 50, 16, 14), (33, 0, 1, 1)):
            x, y, w, h = roi
            assert (pm.motion_pyramid(prev, curr, *params, roi=roi) == whole[y:y + h, x:x + w]).all(), (params, roi)


def test_parameter_bounds():
    assert pm.parameters_ok(2, 16, 2) and pm.parameters_ok(4, 7, 1) and pm.parameters_ok(1, 32, 4)
    assert 16 * 4 + 2 * 3 == 70                          # the defaults' range
    assert not pm.parameters_ok(2, 31, 2)                # range 130
    for bad in ((0, 16, 2), (5, 1, 1), (2, 0, 2), (2, 33, 2), (2, 16, 0), (2, 16, 5)):
        assert not pm.parameters_ok(*bad)


def test_library_exports_the_pyramid_entry_points():
    import __graft_entry__ as entry
    from linux_fg_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        entry.build()
    lib = capi.load()
    for name in ("lfg_motion_pyramid", "lfg_set_motion_estimator"):
        assert getattr(lib, name) is not None
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if " T " in l}
    assert {"lfg_motion_pyramid", "lfg_set_motion_estimator"} <= exported
    assert (capi.ESTIMATOR_FULL_SEARCH, capi.ESTIMATOR_PYRAMID) == (0, 1)
    # no context: refused, nothing else happens
    assert lib.lfg_motion_pyramid(None, None, None, None, 2, 16, 2) != 0
    assert lib.lfg_set_motion_estimator(None, 1) != 0
