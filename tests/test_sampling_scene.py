"""What tests/cases.py: sampling_scene is held to, from the CPU reference alone: the GPU tests of lfg_interpolate_scale
(tests/test_gpu_interpolate_scale.py) compare kernels on it, and a scene whose generated frame is black, or equal to the one
zero vectors give, or the same under both semantics, would let a wrong kernel pass.  These are conditions on the inputs, not
measurements.  CPU only."""
import numpy as np
import pytest

from oracle import scale_f64 as f64
from tests import cases

SHAPES = [wh for wh in f64.sweep_2x_shapes() if wh[0] * wh[1] >= 256] + [(1920, 1080)]


@pytest.mark.parametrize("t", cases.SAMPLING_FACTORS)
@pytest.mark.parametrize("wh", SHAPES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_sampling_scene_samples(oracle, wh, t):
    w, h = wh
    prev, curr, mv = cases.sampling_scene_of(w, h)
    mvf = mv.astype(np.float32)
    mids = []
    for sem in (oracle.REFERENCE, oracle.INTENDED):
        mid = oracle.interpolate(prev, curr, mvf, t, semantics=sem)
        still = oracle.interpolate(prev, curr, np.zeros_like(mvf), t, semantics=sem)
        moved = float((mid != still).any(-1).mean())
        lit = float(mid.any(-1).mean())
        V = f64.scale_f64(mid, 2 * w, 2 * h)
        ties = float(f64.near_half(V, 1e-3).mean())
        print(f"{w}x{h} t={t} semantics {sem}: {moved:.1%} of pixels differ from the zero-vector frame, {lit:.1%} non-black, "
              f"{ties:.3%} near-ties at 2x")
        assert moved >= 0.25
        if sem == oracle.REFERENCE:
            assert 0.20 <= lit <= 0.80
        assert ties <= 0.01
        mids.append(mid)
    assert (mids[0] != mids[1]).any()
