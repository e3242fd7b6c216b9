"""Every frame-taking call of include/linuxfg_hip.h with one operand a view that spans more than 2 GiB or more than 4 GiB
(tests/big_views.py), byte for byte against the model the suite already holds that call to on ordinary frames.

One device allocation per module; every big view starts 2^31 bytes into it, exactly one operand of a call is a big view and all
the others are ordinary small frames.  Inputs are seeded noise, output rows and the 64 bytes to their right hold a sentinel
before the call, and the test moves a big view's rows through tight one-row views only, so neither a misaddressed read nor a
misaddressed store nor a stale result can pass.  The models are computed once per call and shared by every geometry and every
big operand.  tests/big_views.py holds the table of calls and operands (OPERANDS) and says what a geometry leaves out.

An lfg_frame with a pitch above 0x7fffffff (geometry pitch31) must be refused with LFG_ERR_INVALID by every call, with every
output untouched; a mask and an NV12 plane with such a pitch must give the model's bytes.

Offsets kept in pixels or words wrap only at 8 to 16 GiB: spans of that size are out of scope."""
import ctypes
import functools
import re
from collections import namedtuple

import numpy as np
import pytest

from linux_fg_amd import capi
from oracle import scale_f64 as f64
from tests import big_views as bv
from tests.gpu_kit import DEFAULT, apply, assert_matches_f64, ctx

pytestmark = pytest.mark.gpu

W, H = bv.IMAGE
MS, TOL = capi.DEFAULT_MATCH_SAD, 1
FMT = {"rgba": capi.FORMAT_RGBA8, "mv": capi.FORMAT_MV_S8X2, "mvq": capi.FORMAT_MV_S16X2_Q2}
Plane = namedtuple("Plane", "data pitch")           # a mask or an NV12 plane: the runner makes the lfg_mask / lfg_nv12 of it
Built = namedtuple("Built", "inputs run model check", defaults=(None,))


@pytest.fixture(scope="module")
def arena(ctx):
    a = bv.Arena(ctx)
    if a.base is None:
        pytest.skip(f"{a.free} bytes of device memory free, the arena needs {bv.ARENA + 2 ** 30}")
    yield a
    ctx.sync()
    a.release()


@pytest.fixture(autouse=True)
def _settings_restored(ctx):
    yield
    apply(ctx, DEFAULT)
    ctx.set_hole_reach(-1)
    ctx.set_fused_interpolate_scale(False)


# ---- scenes: seeded, so a read from a wrong row cannot return the right texel

def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def moving(w, h):
    """(prev, curr, fwd, bwd): a uniform pan that matches, a block of independent noise in curr and a block of random vectors
    in each field: matched pixels, unmatched ones, collisions and holes."""
    from tests import cases
    prev, curr, fwd = cases.field("uniform", w, h, 7)
    rng = np.random.default_rng(11)
    curr = curr.copy()
    curr[h // 2:, : w // 4] = rng.integers(0, 256, (h - h // 2, w // 4, 4), dtype=np.uint8)
    fwd, bwd = fwd.copy(), (-fwd).astype(np.int8)
    fwd[: h // 2, w // 2:] = rng.integers(-12, 13, (h // 2, w - w // 2, 2)).astype(np.int8)
    bwd[h // 4:, w // 3: w // 2] = rng.integers(-128, 128, (h - h // 4, w // 2 - w // 3, 2)).astype(np.int8)
    return prev, curr, fwd, bwd


@functools.lru_cache(maxsize=None)
def pair(w, h):
    from tests import cases
    return cases.small_scene(w, h, 5)


def quarter(w, h):
    from tests import subpel_model as sp
    prev, curr, fwd, _ = moving(w, h)
    return sp.refine(prev, curr, fwd, 1)


def a_mask(w, h):
    return np.where(np.random.default_rng(13).random((h, w)) < 0.2, np.arange(w, dtype=np.uint8) | 1, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def taps(filt, n_in, n_out):
    return capi.resample_taps(filt, n_in, n_out)


# ---- the calls.  build(w, h) -> Built(inputs, run(ctx, handles) -> what the call returns besides its outputs, model() -> the
# outputs and those extras by name, check(name, got, want) where equality is not the comparison)

def scale_to(ow, oh):
    def build(w, h):
        src = noise(w, h, 21)
        V = f64.scale_f64(src, ow, oh)

        def run(ctx, v):
            ctx.scale(v["in"], v["out"])
            return {"kernel": ctx.scale_last_kernel()}

        def check(name, got, want, big):
            if name == "out":
                assert_matches_f64(got, V, what=f"lfg_scale -> {ow}x{oh}")
            else:
                assert got == want == 0, f"lfg_scale took kernel {got} with a view of 2 GiB or more"
        return Built({"in": src}, run, lambda: {"out": np.rint(np.clip(V, 0, 255)).astype(np.uint8), "kernel": 0}, check)
    return build


def build_motion(w, h):
    import oracle
    prev, curr = pair(w, h)

    def run(ctx, v):
        ctx.motion(v["prev"], v["curr"], v["mv"])
    return Built({"prev": prev, "curr": curr}, run, lambda: {"mv": oracle.motion(prev, curr).astype(np.int8)})


def interpolate_of(kind, multi):
    """kind "centre": zero vectors on the centre rows, where the fast path is eligible while the frames are small (reference
    semantics); "random": the sampling scene's vectors (intended semantics)."""
    def build(w, h):
        import oracle
        from tests import cases
        prev, curr, mv = cases.sampling_scene(w, h, 31)
        sem = capi.SEMANTICS_INTENDED if kind == "random" else capi.SEMANTICS_REFERENCE
        if kind == "centre":
            mv = mv.copy()
            mv[h // 4: h - h // 4] = 0
        factors = (0.3, 0.5) if multi else (0.3,)

        def run(ctx, v):
            ctx.set_semantics(sem)
            outs = [v[f"out{i}"] for i in range(len(factors))]
            if multi:
                ctx.interpolate_multi(v["prev"], v["curr"], v["mv"], outs, factors)
            else:
                ctx.interpolate(v["prev"], v["curr"], v["mv"], outs[0], factors[0])

        def model():
            return {f"out{i}": oracle.interpolate(prev, curr, mv.astype(np.float32), t, semantics=sem) for i, t in enumerate(factors)}
        return Built({"prev": prev, "curr": curr, "mv": mv}, run, model)
    return build


def build_interpolate_scale(w, h):
    """With the fused flag on: the fused kernel (2) addresses prev, curr and out with 32-bit byte offsets and must not run
    with one of them big; the vectors are indexed with size_t, and tests/test_gpu_interpolate_scale.py holds the call to
    kernel 2 for big vectors."""
    import oracle
    from tests import cases
    from tests.test_gpu_interpolate_scale import assert_model
    prev, curr, mv = cases.sampling_scene_of(w, h)
    sem, t = capi.SEMANTICS_INTENDED, 0.3
    mid = oracle.interpolate(prev, curr, mv.astype(np.float32), t, semantics=sem)

    def run(ctx, v):
        ctx.set_semantics(sem)
        ctx.set_fused_interpolate_scale(True)
        ctx.interpolate_scale(v["prev"], v["curr"], v["mv"], v["out"], t)
        return {"kernel": ctx.scale_last_kernel()}

    def check(name, got, want, big):
        if name == "out":
            assert_model(got, mid, "lfg_interpolate_scale")
        else:
            assert got in want and (got != 2 or big == "mv"), f"lfg_interpolate_scale took kernel {got} with {big} a view of 2 GiB or more"
    return Built({"prev": prev, "curr": curr, "mv": mv}, run,
                 lambda: {"out": np.zeros((2 * h, 2 * w, 4), np.uint8), "kernel": (0, 1, 2)}, check)


def build_mv_export(w, h):
    mv = np.random.default_rng(41).integers(-128, 128, (h, w, 2)).astype(np.int8)

    def run(ctx, v):
        return {"image": ctx.mv_export_rgba32f(v["mv"])}

    def model():
        img = np.zeros((h, w, 4), np.float32)
        img[..., :2], img[..., 3] = mv, 1.0
        return {"image": img}
    return Built({"mv": mv}, run, model, lambda name, got, want, big: np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32)))


def build_pyramid(w, h):
    from tests import pyramid_model as pm
    prev, curr = pair(w, h)
    return Built({"prev": prev, "curr": curr}, lambda ctx, v: ctx.motion_pyramid(v["prev"], v["curr"], v["mv"], 2, 16, 2),
                 lambda: {"mv": pm.motion_pyramid(prev, curr, 2, 16, 2)})


def build_refine(w, h):
    from tests import refine_model as rm
    prev, curr, fwd, _ = moving(w, h)
    return Built({"prev": prev, "curr": curr, "mv_in": fwd}, lambda ctx, v: ctx.motion_refine(v["prev"], v["curr"], v["mv_in"], v["mv_out"], 1),
                 lambda: {"mv_out": rm.refine(prev, curr, fwd, 1)})


def build_halve(w, h):
    from tests import expand_model as xm
    src = noise(w, h, 43)
    return Built({"src": src}, lambda ctx, v: ctx.frame_halve(v["src"], v["dst"]), lambda: {"dst": xm.halve(src)})


def build_expand(w, h):
    from tests import expand_model as xm
    prev, curr, fwd, _ = moving(w, h)
    low = np.ascontiguousarray(fwd[::2, ::2] // 2)
    return Built({"prev": prev, "curr": curr, "mv_low": low}, lambda ctx, v: ctx.motion_expand(v["prev"], v["curr"], v["mv_low"], v["mv_out"], 1),
                 lambda: {"mv_out": xm.expand(prev, curr, low, 1)})


def build_subpel(w, h):
    from tests import subpel_model as sp
    prev, curr, fwd, _ = moving(w, h)
    return Built({"prev": prev, "curr": curr, "mv_in": fwd}, lambda ctx, v: ctx.motion_subpel(v["prev"], v["curr"], v["mv_in"], v["mvq"], 1),
                 lambda: {"mvq": sp.refine(prev, curr, fwd, 1)})


def compensated_of(kind, t=0.3):
    """The compensated family: each kind's call and its model on moving()."""
    def build(w, h):
        from tests import bicubic_model as bc, bidir_model as bm, extrapolate_model as ex, fill_model as fm, mc_model as mc
        from tests import overlay_model as ov, subpel_model as sp
        prev, curr, fwd, bwd = moving(w, h)
        inputs = {"prev": prev, "curr": curr, "mv": fwd}
        if kind == "plain":
            run = lambda ctx, v: ctx.interpolate_compensated(v["prev"], v["curr"], v["mv"], v["out"], t, MS)
            want = lambda: mc.interpolate_compensated(prev, curr, fwd, t, MS)
        elif kind == "reach32":
            def run(ctx, v):
                ctx.set_hole_reach(32)
                ctx.interpolate_compensated(v["prev"], v["curr"], v["mv"], v["out"], t, MS)
            want = lambda: fm.interpolate_compensated(prev, curr, fwd, t, 32, MS)
        elif kind == "masked":
            mask = a_mask(w, h)
            inputs["mask"] = mask
            run = lambda ctx, v: ctx.interpolate_compensated_masked(v["prev"], v["curr"], v["mv"], mask_of(v["mask"], w, h), v["out"], t, MS)
            want = lambda: ov.interpolate_masked(prev, curr, fwd, mask, t, MS)
        elif kind == "bidirectional":
            inputs["bwd"] = bwd
            run = lambda ctx, v: ctx.interpolate_compensated_bidirectional(v["prev"], v["curr"], v["mv"], v["bwd"], v["out"], t, MS, TOL)
            want = lambda: bm.interpolate_bidirectional(prev, curr, fwd, bwd, t, MS, TOL)
        elif kind == "extrapolate":
            run = lambda ctx, v: ctx.extrapolate_compensated(v["prev"], v["curr"], v["mv"], v["out"], 0.5, MS)
            want = lambda: ex.extrapolate(prev, curr, fwd, 0.5, MS)
        elif kind == "subpel":
            mvq = inputs["mv"] = quarter(w, h)
            run = lambda ctx, v: ctx.interpolate_compensated_subpel(v["prev"], v["curr"], v["mv"], v["out"], t, MS)
            want = lambda: sp.interpolate(prev, curr, mvq, t, MS)
        else:
            assert kind in ("bicubic", "bicubic_q2"), kind
            field = inputs["mv"] = quarter(w, h) if kind == "bicubic_q2" else fwd
            run = lambda ctx, v: ctx.interpolate_compensated_sampled(v["prev"], v["curr"], v["mv"], v["out"], t, MS, capi.SAMPLING_BICUBIC)
            want = lambda: bc.interpolate(prev, curr, field, t, MS)
        return Built(inputs, run, lambda: {"out": want()})
    return build


def mask_of(p, w, h):
    return capi.Mask(p.data, w, h, p.pitch)


def build_static_mask(w, h):
    from tests import overlay_model as ov
    prev = noise(w, h, 51)
    curr = prev.copy()
    change = np.random.default_rng(52).random((h, w)) < 0.5
    curr[change] ^= 0x10
    return Built({"prev": prev, "curr": curr}, lambda ctx, v: ctx.static_mask(v["prev"], v["curr"], mask_of(v["mask"], w, h), 8),
                 lambda: {"mask": ov.static_mask(prev, curr, 8)})


def build_consistency(w, h):
    from tests import bidir_model as bm
    _, _, fwd, bwd = moving(w, h)
    return Built({"a": fwd, "b": bwd}, lambda ctx, v: ctx.motion_consistency(v["a"], v["b"], TOL, mask_of(v["mask"], w, h)),
                 lambda: {"mask": bm.consistency(fwd, bwd, TOL)})


def build_fill_plane(w, h):
    from tests import fill_cases as fc, fill_model as fm
    K = fc.random_keys(w, h, 6, seed=3)
    words = np.ascontiguousarray(K, np.uint32).view(np.uint8).reshape(h, w, 4)
    return Built({"keys": words}, lambda ctx, v: ctx.hole_fill_plane(v["keys"], v["plane"], 32, False),
                 lambda: {"plane": np.ascontiguousarray(fm.plane(K, 32, False), np.uint32).view(np.uint8).reshape(h, w, 4)})


def build_pair_match(w, h):
    from tests import pair_model
    prev, curr, fwd, _ = moving(w, h)

    def run(ctx, v):
        r = ctx.create_pair_record()
        try:
            ctx.write_pair_record(r, 1, 2, 3)
            ctx.pair_match(v["prev"], v["curr"], v["mv"], r, MS)
            return {"record": ctx.read_pair_record(r)}
        finally:
            ctx.destroy_frame(r)
    return Built({"prev": prev, "curr": curr, "mv": fwd}, run, lambda: {"record": pair_model.pair_stats(prev, curr, fwd, MS)})


def build_cut_fallback(w, h):
    from tests import pair_model
    prev, curr = noise(w, h, 61), noise(w, h, 62)
    factors = (0.25, 0.75)

    def run(ctx, v):
        r = ctx.create_pair_record()
        try:
            ctx.write_pair_record(r, w * h, 0, 0)                 # nothing matched: a cut under any threshold above 0
            ctx.cut_fallback(v["prev"], v["curr"], r, 500, [v["out0"], v["out1"]], factors)
            ctx.sync()
        finally:
            ctx.destroy_frame(r)
    return Built({"prev": prev, "curr": curr}, run, lambda: dict(zip(("out0", "out1"), pair_model.fallback(prev, curr, factors))))


def record_of(which):
    def build(w, h):
        from tests import diff_model as dm, ssim_model as sm
        a = noise(w, h, 71)
        b = np.clip(a.astype(np.int16) + np.random.default_rng(72).integers(-9, 10, a.shape), 0, 255).astype(np.uint8)

        def run(ctx, v):
            r = ctx.create_diff_record() if which == "diff" else ctx.create_ssim_record()
            try:
                ctx.upload(r, np.full((1, r.width, 4), 0xFF, np.uint8))
                if which == "diff":
                    ctx.frame_diff(v["a"], v["b"], r)
                    return {"record": ctx.read_diff_record(r)}
                ctx.frame_ssim(v["a"], v["b"], r)
                return {"record": ctx.read_ssim_record(r)}
            finally:
                ctx.destroy_frame(r)
        return Built({"a": a, "b": b}, run, lambda: {"record": dm.frame_diff(a, b) if which == "diff" else sm.frame_ssim(a, b)})
    return build


def nv12_of(v, w, h):
    return capi.Nv12(v["y"].data, v["uv"].data, w, h, v["y"].pitch, v["uv"].pitch)


def yuv_of(direction, siting):
    def build(w, h):
        from tests import yuv_model as ym
        mode = (ym.BT709, ym.LIMITED, siting)
        if direction == "to_rgba":
            y, uv = ym.random_nv12(w, h, 81)
            return Built({"y": y, "uv": uv.reshape(h // 2, w)}, lambda ctx, v: ctx.nv12_to_rgba(nv12_of(v, w, h), v["rgba"], *mode),
                         lambda: {"rgba": ym.nv12_to_rgba(y, uv, *mode)})
        rgba = ym.random_rgba(w, h, 82)

        def model():
            wy, wuv = ym.rgba_to_nv12(rgba, *mode)
            return {"y": wy, "uv": wuv.reshape(h // 2, w)}
        return Built({"rgba": rgba}, lambda ctx, v: ctx.rgba_to_nv12(v["rgba"], nv12_of(v, w, h), *mode), model)
    return build


def build_sharpen(w, h):
    from tests import sharpen_model as shm
    src = shm.noise(w, h, 91)
    return Built({"src": src}, lambda ctx, v: ctx.sharpen(v["src"], v["dst"], 37), lambda: {"dst": shm.sharpen(src, 37)})


def resample_to(ow, oh, strength=None, src=None):
    def build(w, h):
        w, h = src or (w, h)
        from tests import antiring_model as am, resample_model as rsm
        frame, filt = noise(w, h, 95), capi.FILTER_LANCZOS3
        tx, ty = taps(filt, w, ow), taps(filt, h, oh)
        if strength is None:
            return Built({"src": frame}, lambda ctx, v: ctx.resample(v["src"], v["dst"], filt), lambda: {"dst": rsm.resample_int(frame, tx, ty)})
        return Built({"src": frame}, lambda ctx, v: ctx.resample_antiring(v["src"], v["dst"], filt, strength),
                     lambda: {"dst": am.antiring(frame, ow, oh, filt, strength, tx, ty)})
    return build


def transfer_of(which):
    """lfg_frame_copy, lfg_frame_upload, lfg_frame_download and the ring's two transfers: the bytes arrive unchanged."""
    def build(w, h):
        data = noise(w, h, 97)

        def ring(ctx, frame, upload):
            lib, r, host, slot = ctx.lib, ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
            assert lib.lfg_ring_create(ctx.h, 2, data.nbytes, ctypes.byref(r)) == 0
            try:
                assert lib.lfg_ring_acquire(r, ctypes.byref(host), ctypes.byref(slot)) == 0
                pinned = np.ctypeslib.as_array((ctypes.c_uint8 * data.nbytes).from_address(host.value))
                pinned[:] = data.reshape(-1) if upload else 0x3C
                rc = (lib.lfg_ring_upload if upload else lib.lfg_ring_download)(r, slot, ctypes.byref(frame))
                if rc != 0:
                    raise capi.LfgError(f"lfg_ring transfer failed ({rc}): {lib.lfg_last_error(ctx.h).decode()}")
                assert lib.lfg_ring_wait(r, slot) == 0
                ctx.sync()
                return pinned.reshape(data.shape).copy()
            finally:
                lib.lfg_ring_destroy(r)

        if which == "copy":
            return Built({"src": data}, lambda ctx, v: ctx.copy(v["src"], v["dst"]), lambda: {"dst": data})
        if which == "upload":
            return Built({}, lambda ctx, v: ctx.upload(v["dst"], data), lambda: {"dst": data})
        if which == "download":
            return Built({"src": data}, lambda ctx, v: {"host": ctx.download(v["src"])}, lambda: {"host": data})
        if which == "ring_upload":
            return Built({}, lambda ctx, v: (ring(ctx, v["dst"], True), None)[1], lambda: {"dst": data})
        assert which == "ring_download", which
        return Built({"src": data}, lambda ctx, v: {"host": ring(ctx, v["src"], False)}, lambda: {"host": data})
    return build


FRAMES_SETTINGS = {"default": (DEFAULT, False), "fused": (DEFAULT, True), "pyramid_compensated": (("pyramid", -1, "compensated", capi.SEMANTICS_INTENDED), False)}


@functools.lru_cache(maxsize=None)
def chain_of(w, h):
    from tests import route_cases
    return route_cases.RouteChain(*pair(w, h))


def frames_of(setting, multi):
    """lfg_interpolate_frames[_multi] under the default, the fused order (the FusedOut store) and pyramid + compensated."""
    def build(w, h):
        from tests import route_cases
        prev, curr = pair(w, h)
        tuple4, fused = FRAMES_SETTINGS[setting]
        factors = (0.25, 0.5) if multi else (0.5,)

        def run(ctx, v):
            apply(ctx, tuple4, fused=fused)
            outs = [v[f"out{i}"] for i in range(len(factors))]
            if multi:
                ctx.interpolate_frames_multi(v["prev"], v["curr"], outs, factors)
            else:
                ctx.interpolate_frames(v["prev"], v["curr"], outs[0], factors[0])

        def model():
            return dict((f"out{i}", f) for i, f in enumerate(chain_of(w, h).frames(route_cases.route(tuple4, fused=fused), factors)))
        return Built({"prev": prev, "curr": curr}, run, model)
    return build


# name -> (build, the operands of bv.OPERANDS[name])
BUILD = {
    "scale_2x": scale_to(2 * W, 2 * H), "scale_generic": scale_to(96, 60), "motion": build_motion,
    "interpolate_centre": interpolate_of("centre", False), "interpolate_random": interpolate_of("random", False),
    "interpolate_multi_centre": interpolate_of("centre", True), "interpolate_multi_random": interpolate_of("random", True),
    "interpolate_scale": build_interpolate_scale, "mv_export": build_mv_export, "motion_pyramid": build_pyramid,
    "motion_refine": build_refine, "frame_halve": build_halve, "motion_expand": build_expand, "motion_subpel": build_subpel,
    "compensated": compensated_of("plain"), "compensated_reach32": compensated_of("reach32"), "masked": compensated_of("masked"),
    "bidirectional": compensated_of("bidirectional"), "extrapolate": compensated_of("extrapolate"), "subpel": compensated_of("subpel"),
    "bicubic": compensated_of("bicubic"), "bicubic_q2": compensated_of("bicubic_q2"), "static_mask": build_static_mask,
    "motion_consistency": build_consistency, "hole_fill_plane": build_fill_plane, "pair_match": build_pair_match,
    "cut_fallback": build_cut_fallback, "frame_diff": record_of("diff"), "frame_ssim": record_of("ssim"),
    "nv12_to_rgba_left": yuv_of("to_rgba", capi.CHROMA_LEFT), "nv12_to_rgba_replicate": yuv_of("to_rgba", capi.CHROMA_REPLICATE),
    "rgba_to_nv12_left": yuv_of("to_nv12", capi.CHROMA_LEFT), "rgba_to_nv12_replicate": yuv_of("to_nv12", capi.CHROMA_REPLICATE),
    "sharpen": build_sharpen, "resample_up": resample_to(96, 60), "resample_down": resample_to(*bv.DOWN[1], src=bv.DOWN[0]),
    "resample_antiring": resample_to(96, 60, strength=48), "frame_copy": transfer_of("copy"), "frame_upload": transfer_of("upload"),
    "frame_download": transfer_of("download"), "ring_upload": transfer_of("ring_upload"), "ring_download": transfer_of("ring_download"),
}
BUILD.update({f"frames_{s}": frames_of(s, False) for s in FRAMES_SETTINGS})
BUILD.update({f"frames_multi_{s}": frames_of(s, True) for s in FRAMES_SETTINGS})
assert set(BUILD) == set(bv.OPERANDS), set(BUILD) ^ set(bv.OPERANDS)


@functools.lru_cache(maxsize=None)
def built(name, w, h):
    b = BUILD[name](w, h)
    return b, b.model()


# ---- one case

def as_rows(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def code_of(call):
    """0, or the status the binding's LfgError carries."""
    try:
        return 0, call()
    except capi.LfgError as e:
        return int(re.search(r"failed \((-?\d+)\)", str(e)).group(1)), None


def run_case(ctx, arena, name, big, geometry, w, h):
    """One call with `big` as the view of `geometry`.  A HIP-level error ends the session: nothing more is started on that GPU."""
    try:
        _run_case(ctx, arena, name, big, geometry, w, h)
    except capi.LfgError as e:
        if "(-2)" in str(e):
            pytest.exit(f"{name}, {big} {geometry}: {e}", returncode=3)
        raise


def _run_case(ctx, arena, name, big, geometry, w, h):
    b, want = built(name, w, h)
    operands = bv.operands_of(name, w, h)
    refused = geometry == "pitch31" and operands[big].kind in FMT
    views, owned, outputs = {}, [], {}
    try:
        for op, (kind, role, rows, n) in operands.items():
            data = as_rows(b.inputs[op]) if role == "in" else np.full((rows, n), bv.SENTINEL, np.uint8)
            assert data.shape == (rows, n), (op, data.shape, rows, n)
            if op == big:                           # (a refused view reaches beyond the arena: its first two rows are staged)
                address, pitch = arena.view, bv.pitch_of(geometry, rows, bv.PLANE[kind])
                assert refused or bv.fits(geometry, rows, n, bv.PLANE[kind])
                bv.write_rows(ctx, address, pitch, data[:2] if refused else data, right=bv.GUARD if role == "out" else 0)
            else:                                   # an ordinary tight frame; the guard follows its last row
                f = ctx.create_frame((rows * n + bv.GUARD) // 4 + 2, 1)
                owned.append(f)
                address, pitch = f.data, n
                bv.write_rows(ctx, address, rows * n, data.reshape(1, -1), right=bv.GUARD)
            if role == "out":
                outputs[op] = (address, pitch, rows, n)
            if kind in FMT:
                ow = n // capi._BPP[FMT[kind]]
                views[op] = (capi.Frame(address, ow, rows, pitch, FMT[kind], 0, 0) if refused and op == big
                             else capi.Context.wrap(address, ow, rows, FMT[kind], pitch=pitch))
            else:
                views[op] = Plane(address, pitch)
        rc, extras = code_of(lambda: b.run(ctx, views))
        if rc == -2:
            pytest.exit(f"{name}, {big} {geometry}: {ctx.lib.lfg_last_error(ctx.h).decode()}", returncode=3)
        ctx.sync()
        what = f"{name}, {big} {geometry}"
        if refused:
            assert rc == capi.ERR_INVALID, f"{what}: status {rc}, not LFG_ERR_INVALID"
        else:
            assert rc == 0, f"{what}: status {rc}: {ctx.lib.lfg_last_error(ctx.h).decode()}"
        for op, (address, pitch, rows, n) in outputs.items():
            if op == big:
                got, right = bv.read_rows(ctx, address, pitch, 2 if refused else rows, n, bv.GUARD)
            else:
                got, right = bv.read_rows(ctx, address, rows * n, 1, rows * n, bv.GUARD)
                got = got.reshape(rows, n)
            assert (right == bv.SENTINEL).all(), f"{what}: bytes to the right of {op}'s rows were written"
            if refused:
                assert (got == bv.SENTINEL).all(), f"{what}: {op} was written by a call that refused"
                continue
            model = np.ascontiguousarray(want[op])
            got = got.copy().view(model.dtype).reshape(model.shape)
            if b.check:
                b.check(op, got, model, big)
            else:
                bad = np.argwhere(as_rows(got) != as_rows(model))
                assert not len(bad), f"{what}: {op} differs from the model in {len(bad)} bytes, first (row, byte) {bad[:4].tolist()}"
        if not refused:
            for key in set(want) - set(outputs):
                if b.check:
                    b.check(key, extras[key], want[key], big)
                else:
                    same = np.array_equal(extras[key], want[key]) if isinstance(want[key], np.ndarray) else extras[key] == want[key]
                    assert same, f"{what}: {key} {extras[key]} against the model's {want[key]}"
    finally:
        for f in owned:
            ctx.destroy_frame(f)


@pytest.mark.parametrize("name,big,geometry", bv.tall_cases(), ids=["-".join(c) for c in bv.tall_cases()])
def test_one_operand_spans_2_or_4_gib(ctx, arena, oracle, name, big, geometry):
    run_case(ctx, arena, name, big, geometry, W, H)


@pytest.mark.parametrize("name,big", bv.frame_operands(), ids=["-".join(c) for c in bv.frame_operands()])
def test_a_frame_pitch_above_int_max_is_refused(ctx, arena, oracle, name, big):
    """The lfg_frame is made by hand: lfg_frame_wrap refuses it too."""
    f = capi.Frame()
    assert ctx.lib.lfg_frame_wrap(ctypes.c_void_p(arena.view), W, 2, 2 ** 31 + 64, capi.FORMAT_RGBA8, ctypes.byref(f)) == capi.ERR_INVALID
    run_case(ctx, arena, name, big, "pitch31", W, H)


@pytest.mark.parametrize("name,big,w,h", bv.plane_cases(), ids=["-".join(map(str, c)) for c in bv.plane_cases()])
def test_a_plane_pitch_above_int_max_is_exact(ctx, arena, oracle, name, big, w, h):
    """A mask, a luma plane and a chroma plane of two rows, 2^31 + 64 bytes apart: the kernels take these pitches as size_t."""
    run_case(ctx, arena, name, big, "pitch31", w, h)
