"""What the GPU test files share.  `ctx` is a pytest fixture: a test file imports it by name, which makes it that module's own
(one context per file, as when each file defined it), and a linter will call that import unused."""
import json
import os
import subprocess

import numpy as np
import pytest

from linux_fg_amd import capi
from oracle import scale_f64 as f64
from tests.host_cli import HOST, ROOT, built


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


_host_failed = None                                # why no further lfg_host is started in this session


def host_run(tmp_path, frames, out_size, *options, timeout=300):
    """`frames` through lfg_host as a raw file, presented at out_size = (width, height) under `options`, which say everything
    else -- the semantics and the formats included: (its report line, the frames it presented).  With --input-format nv12 among
    the options each frame is (y, uv), else an (h, w, 4) array; with --output-format nv12 the presented frames come back as a
    list of (y, uv), else as one (presented, height, width, 4) array.

    A run that times out or dies from a signal may have left the GPU in a state in which the next run does the same: the first
    such run fails its test, and every later call fails at once without starting lfg_host again."""
    global _host_failed
    if _host_failed:
        pytest.fail(f"lfg_host is not started again in this session: {_host_failed}", pytrace=False)
    built(HOST)
    options = [str(o) for o in options]

    def fmt(name):
        at = [i for i, o in enumerate(options) if o == name]
        return options[at[-1] + 1] if at else "rgba"

    nv12_in, nv12_out = fmt("--input-format") == "nv12", fmt("--output-format") == "nv12"
    (h, w), (ow, oh) = (frames[0][0].shape if nv12_in else frames[0].shape[:2]), out_size
    tmp_path.mkdir(exist_ok=True)
    src, out = tmp_path / ("in.nv12" if nv12_in else "in.rgba"), tmp_path / ("out.nv12" if nv12_out else "out.rgba")
    np.concatenate([np.asarray(part).reshape(-1) for f in frames for part in (f if nv12_in else (f,))]).tofile(src)
    command = [HOST, "--input-width", str(w), "--input-height", str(h), "--output-width", str(ow), "--output-height", str(oh),
               "--frames", str(len(frames)), "--quiet", "--input-raw", str(src), "--output-raw", str(out), *options]
    try:
        p = subprocess.run(command, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _host_failed = f"a run did not end within {timeout} s ({' '.join(options)})"
        pytest.fail(_host_failed, pytrace=False)
    if p.returncode < 0:
        _host_failed = f"a run died from signal {-p.returncode} ({' '.join(options)})"
        pytest.fail(_host_failed + "\n" + p.stderr[-2000:], pytrace=False)
    assert p.returncode == 0, p.stderr
    info = json.loads(p.stdout.strip().splitlines()[-1])
    raw = np.fromfile(out, np.uint8)
    each = ow * oh * 3 // 2 if nv12_out else ow * oh * 4
    assert raw.size == info["presented"] * each, (raw.size, info["presented"], each)
    if not nv12_out:
        return info, raw.reshape(info["presented"], oh, ow, 4)
    return info, [(f[:ow * oh].reshape(oh, ow), f[ow * oh:].reshape(oh // 2, ow // 2, 2)) for f in raw.reshape(info["presented"], each)]


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
