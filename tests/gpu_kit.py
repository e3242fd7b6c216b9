"""What the GPU test files share.  `ctx` is a pytest fixture: a test file imports it by name, which makes it that module's own
(one context per file, as when each file defined it), and a linter will call that import unused."""
import json
import os
import subprocess

import numpy as np
import pytest

from linux_fg_amd import capi
from oracle import scale_f64 as f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "linux-fg_amd", "lfg_host")


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as entry
    if not os.path.exists(capi.LIB_PATH):
        entry.build()
    with capi.Context(0) as c:
        yield c


ESTIMATOR = {"full": capi.ESTIMATOR_FULL_SEARCH, "pyramid": capi.ESTIMATOR_PYRAMID}
INTERPOLATOR = {"shader": capi.INTERPOLATOR_SHADER, "compensated": capi.INTERPOLATOR_COMPENSATED}
DEFAULT = ("full", -1, "shader", capi.SEMANTICS_REFERENCE)


def apply(ctx, setting, fused=False, match_sad=capi.DEFAULT_MATCH_SAD, threshold=-1):
    """The setters a host calls for setting = (estimator, refinement radius, interpolator, semantics), the fused order and
    cut detection, which is set to off (-1) unless a threshold is given.  None of them waits for the GPU."""
    estimator, radius, interpolator, semantics = setting
    ctx.set_motion_estimator(ESTIMATOR[estimator])
    ctx.set_vector_refinement(radius)
    ctx.set_interpolator(INTERPOLATOR[interpolator], match_sad)
    ctx.set_semantics(semantics)
    ctx.set_fused_motion_interpolate(fused)
    ctx.set_cut_detection(threshold)


def gpu_vectors(ctx, prev, curr, estimator):
    """The vectors of "full" (lfg_motion) or "pyramid" (lfg_motion_pyramid at 2, 16, 2) under the intended semantics."""
    h, w = prev.shape[:2]
    p, c = ctx.frame_from(prev), ctx.frame_from(curr)
    m = ctx.create_frame(w, h, capi.FORMAT_MV_S8X2)
    ctx.set_semantics(capi.SEMANTICS_INTENDED)
    try:
        if estimator == "full":
            ctx.motion(p, c, m)
        else:
            ctx.motion_pyramid(p, c, m, 2, 16, 2)
        return ctx.download(m)
    finally:
        ctx.set_semantics(capi.SEMANTICS_REFERENCE)
        for f in (p, c, m):
            ctx.destroy_frame(f)


def pitched(ctx, host, pad_px, fmt=capi.FORMAT_RGBA8):
    """`host` in the left part of a wider frame, described with the wider row pitch (lfg_frame_wrap), as a caller handing
    over a sub-rectangle would; the padding poisoned with 0x5A bytes.  Returns (the wider frame, the view)."""
    h, w, ch = host.shape
    wide = np.full((h, w + pad_px, ch), 0x5A, host.dtype)
    wide[:, :w] = host
    big = ctx.frame_from(wide, fmt)
    return big, capi.Context.wrap(big.data, w, h, fmt, pitch=(w + pad_px) * ch)


def first_bad(got, want):
    bad = np.argwhere((got != want).any(-1))
    return f"{len(bad)} pixels differ, first {bad[:3].tolist()}"


def assert_matches_f64(got, V, eps=1e-3, what=""):
    """The kernel's bytes against the float64 model's unrounded values V (oracle/scale_f64.py): within half an LSB plus
    eps everywhere, and exactly rint(clip(V)) wherever V is further than eps from a rounding boundary.  The kernels'
    fp32 arithmetic stays within ~1e-4 LSB of V, so this is ~500 times tighter than +-1 LSB; with the bound on the
    shader (tests/test_scale_model.py) it gives +-1 LSB against the shader for every input.  Returns the near-ties."""
    c = np.clip(V, 0.0, 255.0)
    d = np.abs(got.astype(np.float64) - c)
    at = tuple(int(i) for i in np.unravel_index(d.argmax(), d.shape))
    assert d.max() <= 0.5 + eps, f"{what}: |got - V| = {d.max():.5f} at {at} (got {got[at]}, V {V[at]:.5f})"
    near = f64.near_half(V, eps)
    bad = ~near & (got != np.rint(c))
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} bytes differ from rint(V) away from a tie, "
                             f"first at {at} (got {got[at]}, V {V[at]:.5f})")
    ties = int(near.sum())
    print(f"f64 model {what}: {ties} near-ties in {got.size} bytes")
    return ties


def seam_rows(in_h):
    """Input rows that straddle the 2x kernel's strip and XCD-band seams: an impulse at row first - 3 of a strip
    reaches the last output rows of the strip above it and the first of its own."""
    import ctypes
    lib = capi.load()
    per, first, steps = ctypes.c_uint32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.lfg_diag_scale_2x_strip(in_h, 0, 0, ctypes.byref(per), None, None) == 0
    rows = set()
    for x in range(8):
        for i in range(per.value):
            assert lib.lfg_diag_scale_2x_strip(in_h, x, i, None, ctypes.byref(first), ctypes.byref(steps)) == 0
            if steps.value > 0:
                rows.add(first.value - 3)
    return sorted(r for r in rows if 0 <= r < in_h)


def host_stream(tmp_path, frames, *options):
    """`frames` through lfg_host as a raw file, under the intended semantics and `options`: (its report line, the 2 n - 1
    frames it presents)."""
    if not os.path.exists(HOST):
        import __graft_entry__ as entry
        entry.build()
    n, (h, w) = len(frames), frames[0].shape[:2]
    tmp_path.mkdir(exist_ok=True)
    src, out = tmp_path / "in.rgba", tmp_path / "out.rgba"
    np.concatenate([f.reshape(-1) for f in frames]).tofile(src)
    p = subprocess.run([HOST, "--input-width", str(w), "--input-height", str(h), "--frames", str(n), "--quiet",
                        "--input-raw", str(src), "--output-raw", str(out), "--semantics", "intended", *options],
                       capture_output=True, text=True, timeout=300, check=True)
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["presented"] == 2 * n - 1
    return info, np.fromfile(out, np.uint8).reshape(2 * n - 1, h, w, 4)


def three_lanes(ctx, inputs, enqueue, alone):
    """Input i on lane i % 3, everything enqueued before the one sync.  enqueue(i, *inputs[i]) uploads what the call reads,
    makes the call and returns its frames, the output last: each output must be alone[i], what the call gave on one lane."""
    ctx.lanes(3)
    try:
        frames = []
        for i, arrays in enumerate(inputs):
            ctx.lane_select(i % 3)
            frames.append(enqueue(i, *arrays))
        ctx.sync()
        for fs, want in zip(frames, alone):
            assert (ctx.download(fs[-1]) == want).all()
            for f in fs:
                ctx.destroy_frame(f)
    finally:
        ctx.lane_select(0)
        ctx.lanes(1)
