"""ctypes front end of the CPU oracle (oracle/lfg_oracle.c).

TEST INFRASTRUCTURE ONLY -- see the header of lfg_oracle.c.  Only tests/,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg import this
package; the product package (linux-fg_amd/) never does.

The reference cannot run as Vulkan here, but the text of its three shaders can: oracle/ref_recipe.py
compiles it as C++ against oracle/glsl_shim.hpp into oracle/_ref/liblfg_ref.so, and ``ref_scale``, ``ref_motion`` and
``ref_interpolate`` below run it.  tests/test_reference_shaders.py holds the oracle to those, so the oracle's reading of the
shader text is executed; the built-in choices (1)-(7) and (9) of lfg_oracle.c's header and the Vulkan host code are read.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from . import ref_recipe

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "liblfg_oracle.so")
_lib = None

_u8p = ctypes.POINTER(ctypes.c_uint8)
_f32p = ctypes.POINTER(ctypes.c_float)


def build(force: bool = False) -> str:
    """Compile liblfg_oracle.so with gcc if it is missing or older than its source, and bring oracle/_ref/ (the executed
    reference shaders, oracle/ref_recipe.py) up to date where the reference is at hand."""
    src = os.path.join(_HERE, "lfg_oracle.c")
    stale = (not os.path.exists(_LIB_PATH)) or os.path.getmtime(_LIB_PATH) < os.path.getmtime(src)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", _HERE, "-B", "liblfg_oracle.so"])
    ref_recipe.build(force)
    return _LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB_PATH)
        i = ctypes.c_int
        L.lfg_oracle_scale.argtypes = [_u8p, i, i, _u8p, i, i, i, i, i, i, i]
        L.lfg_oracle_scale.restype = i
        L.lfg_oracle_motion.argtypes = [_u8p, _u8p, i, i, i, ctypes.c_float, _f32p, i, i, i, i, i]
        L.lfg_oracle_motion.restype = i
        L.lfg_oracle_interpolate.argtypes = [_u8p, _u8p, _f32p, i, i, ctypes.c_float, _u8p, i, i, i, i, i]
        L.lfg_oracle_interpolate.restype = i
        L.lfg_oracle_motion_ex.argtypes = [_u8p, _u8p, i, i, i, ctypes.c_float, _f32p, i, i, i, i, i, i]
        L.lfg_oracle_motion_ex.restype = i
        L.lfg_oracle_interpolate_ex.argtypes = [_u8p, _u8p, _f32p, i, i, ctypes.c_float, _u8p, i, i, i, i, i, i]
        L.lfg_oracle_interpolate_ex.restype = i
        L.lfg_oracle_lanczos_taps.argtypes = [i, i, i, _f32p]
        L.lfg_oracle_lanczos_taps.restype = i
        _lib = L
    return _lib


def default_threads() -> int:
    """Host threads for the oracle: the affinity mask, capped at 16 (a one-GPU box's CPU share)."""
    cap = int(os.environ.get("LFG_ORACLE_THREADS", "16"))
    return max(1, min(cap, len(os.sched_getaffinity(0))))


def _frame(a: np.ndarray, name: str) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"{name}: expected an (H, W, 4) uint8 RGBA frame, got {a.shape}")
    return a


def _roi(roi, W, H):
    if roi is None:
        return 0, 0, W, H
    x0, y0, x1, y1 = (int(v) for v in roi)
    return x0, y0, x1, y1


def scale(frame: np.ndarray, out_w: int, out_h: int, roi=None, threads: int | None = None) -> np.ndarray:
    """shaders/scale.comp.  Returns an (out_h, out_w, 4) uint8 frame; pixels outside ``roi`` are 0."""
    f = _frame(frame, "frame")
    out = np.zeros((out_h, out_w, 4), np.uint8)
    x0, y0, x1, y1 = _roi(roi, out_w, out_h)
    rc = lib().lfg_oracle_scale(f.ctypes.data_as(_u8p), f.shape[1], f.shape[0],
                                out.ctypes.data_as(_u8p), out_w, out_h, x0, y0, x1, y1,
                                threads or default_threads())
    if rc != 0:
        raise ValueError("lfg_oracle_scale: bad arguments")
    return out


REFERENCE, INTENDED = 0, 1      # semantics: the shaders as written / the opt-in "intended" variant (not the parity contract)


def motion(prev: np.ndarray, curr: np.ndarray, block_size: int = 8, search_radius: float = 16.0,
           roi=None, threads: int | None = None, semantics: int = REFERENCE) -> np.ndarray:
    """shaders/motion.comp.  Returns (H, W, 2) float32 motion vectors (x, y); 0 outside ``roi``.
    ``semantics=INTENDED``: equal costs are broken towards the shortest vector (flat areas give (0,0))."""
    p, c = _frame(prev, "prev"), _frame(curr, "curr")
    if p.shape != c.shape:
        raise ValueError("prev and curr differ in size")
    H, W = p.shape[:2]
    mv = np.zeros((H, W, 2), np.float32)
    x0, y0, x1, y1 = _roi(roi, W, H)
    rc = lib().lfg_oracle_motion_ex(p.ctypes.data_as(_u8p), c.ctypes.data_as(_u8p), W, H, int(block_size),
                                    float(search_radius), mv.ctypes.data_as(_f32p), x0, y0, x1, y1,
                                    threads or default_threads(), int(semantics))
    if rc != 0:
        raise ValueError("lfg_oracle_motion: bad arguments")
    return mv


def interpolate(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray, factor: float = 0.5,
                roi=None, threads: int | None = None, semantics: int = REFERENCE) -> np.ndarray:
    """shaders/interpolate.comp.  ``mv`` is (H, W, 2) float32 in whole pixels (literal semantics, F5).
    ``semantics=INTENDED``: the vector is divided by the image size before it is added to uv."""
    p, c = _frame(prev, "prev"), _frame(curr, "curr")
    if p.shape != c.shape:
        raise ValueError("prev and curr differ in size")
    H, W = p.shape[:2]
    m = np.ascontiguousarray(mv, dtype=np.float32)
    if m.shape != (H, W, 2):
        raise ValueError(f"mv: expected {(H, W, 2)}, got {m.shape}")
    out = np.zeros((H, W, 4), np.uint8)
    x0, y0, x1, y1 = _roi(roi, W, H)
    rc = lib().lfg_oracle_interpolate_ex(p.ctypes.data_as(_u8p), c.ctypes.data_as(_u8p), m.ctypes.data_as(_f32p),
                                         W, H, float(factor), out.ctypes.data_as(_u8p), x0, y0, x1, y1,
                                         threads or default_threads(), int(semantics))
    if rc != 0:
        raise ValueError("lfg_oracle_interpolate: bad arguments")
    return out


def lanczos_taps(p: int, in_size: int, out_size: int):
    """(start index, six raw weights) for output coordinate ``p`` on one axis (scale.comp:24-41)."""
    w = (ctypes.c_float * 6)()
    s = lib().lfg_oracle_lanczos_taps(int(p), int(in_size), int(out_size), w)
    return s, np.array(list(w), np.float32)


# ---- the reference's own shader text, executed (oracle/_ref/, built by oracle/ref_recipe.py)

_ref = None


def ref_available() -> bool:
    """Whether the executed shaders can be called: builds oracle/_ref/ from the reference if it is there, else takes an
    earlier build if there is one."""
    return ref_recipe.build() is not None


def ref_lib() -> ctypes.CDLL:
    global _ref
    if _ref is None:
        path = ref_recipe.build()
        if path is None:
            raise RuntimeError(f"no reference shaders at {ref_recipe.reference_dir()} and no earlier build in oracle/_ref")
        L = ctypes.CDLL(path)
        i = ctypes.c_int
        L.ref_scale.argtypes = [_u8p, i, i, _u8p, i, i, i, i, i, i, i]
        L.ref_motion.argtypes = [_u8p, _u8p, i, i, i, ctypes.c_float, _f32p, _f32p, i, i, i, i, i]
        L.ref_interpolate.argtypes = [_u8p, _u8p, _f32p, i, i, ctypes.c_float, _u8p, _u8p, i, i, i, i, i]
        for f in (L.ref_scale, L.ref_motion, L.ref_interpolate):
            f.restype = i
        _ref = L
    return _ref


def ref_scale(frame: np.ndarray, out_w: int, out_h: int, roi=None, threads: int | None = None) -> np.ndarray:
    """shaders/scale.comp itself, executed.  Same conventions as ``scale``; ``roi`` runs as every 16 x 16 workgroup that
    overlaps it, and only its pixels are stored."""
    f = _frame(frame, "frame")
    out = np.zeros((out_h, out_w, 4), np.uint8)
    x0, y0, x1, y1 = _roi(roi, out_w, out_h)
    rc = ref_lib().ref_scale(f.ctypes.data_as(_u8p), f.shape[1], f.shape[0], out.ctypes.data_as(_u8p), out_w, out_h,
                             x0, y0, x1, y1, threads or default_threads())
    if rc != 0:
        raise ValueError("ref_scale: bad arguments")
    return out


def ref_motion(prev: np.ndarray, curr: np.ndarray, block_size: int = 8, search_radius: float = 16.0,
               roi=None, threads: int | None = None, with_zw: bool = False):
    """shaders/motion.comp itself, executed.  Same conventions as ``motion`` (reference semantics only).  With ``with_zw``
    returns (xy, zw), both (H, W, 2) float32: the two halves of the rgba32f texel the shader stores."""
    p, c = _frame(prev, "prev"), _frame(curr, "curr")
    if p.shape != c.shape:
        raise ValueError("prev and curr differ in size")
    H, W = p.shape[:2]
    mv = np.zeros((H, W, 2), np.float32)
    zw = np.zeros((H, W, 2), np.float32) if with_zw else None
    x0, y0, x1, y1 = _roi(roi, W, H)
    rc = ref_lib().ref_motion(p.ctypes.data_as(_u8p), c.ctypes.data_as(_u8p), W, H, int(block_size), float(search_radius),
                              mv.ctypes.data_as(_f32p), zw.ctypes.data_as(_f32p) if with_zw else None,
                              x0, y0, x1, y1, threads or default_threads())
    if rc != 0:
        raise ValueError("ref_motion: bad arguments")
    return (mv, zw) if with_zw else mv


def ref_interpolate(prev: np.ndarray, curr: np.ndarray, mv: np.ndarray, factor: float = 0.5,
                    roi=None, threads: int | None = None):
    """shaders/interpolate.comp itself, executed.  Same conventions as ``interpolate`` (reference semantics only), but the
    vectors are fetched with texture() as a bilinear sample -- choice (8) of lfg_oracle.c is not made.  Returns (frame, mask):
    mask is (H, W) bool, True where that fetch had a non-zero fractional weight, i.e. where (8) is an assumption."""
    p, c = _frame(prev, "prev"), _frame(curr, "curr")
    if p.shape != c.shape:
        raise ValueError("prev and curr differ in size")
    H, W = p.shape[:2]
    m = np.ascontiguousarray(mv, dtype=np.float32)
    if m.shape != (H, W, 2):
        raise ValueError(f"mv: expected {(H, W, 2)}, got {m.shape}")
    out = np.zeros((H, W, 4), np.uint8)
    mask = np.zeros((H, W), np.uint8)
    x0, y0, x1, y1 = _roi(roi, W, H)
    rc = ref_lib().ref_interpolate(p.ctypes.data_as(_u8p), c.ctypes.data_as(_u8p), m.ctypes.data_as(_f32p), W, H, float(factor),
                                   out.ctypes.data_as(_u8p), mask.ctypes.data_as(_u8p), x0, y0, x1, y1, threads or default_threads())
    if rc != 0:
        raise ValueError("ref_interpolate: bad arguments")
    return out, mask.astype(bool)


def inexact_centres(n: int) -> np.ndarray:
    """(n,) bool: the indices i at which a texel centre, taken through the shaders' own fp32 arithmetic, misses itself --
    fl(fl(fl((i + 0.5) / n) * n) - 0.5) != i, every operation rounded to fp32.  There texture() on the vector image has a
    non-zero fractional weight and choice (8) of lfg_oracle.c is an assumption; everywhere else it is a fact."""
    i = np.arange(n, dtype=np.float32)
    uv = (i + np.float32(0.5)) / np.float32(n)
    return (uv * np.float32(n) - np.float32(0.5)) != i
