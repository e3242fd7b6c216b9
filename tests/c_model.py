"""What the CPU models (pyramid_model.py, mc_model.py, refine_model.py) share: the loader of their C sources, built with the
system C compiler on first use, and the hand-over of numpy arrays to them."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}


def load(name, signatures, flags=(), libs=()):
    """tests/<name>.c as a ctypes library, built with cc -O2 -shared -fPIC `flags` ... `libs`.  `signatures` gives the argtypes
    of its functions (all return void).  The build is cached in the temp directory under a name made from the source and the
    command, so an edited source or another set of flags never loads a stale library; the rename makes a half-written file
    invisible to a test process running next to this one."""
    key = (name, tuple(flags), tuple(libs))
    if key not in _libs:
        src = os.path.join(_HERE, name + ".c")
        cmd = [os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", *flags]
        tag = hashlib.sha1(open(src, "rb").read() + " ".join(cmd + list(libs)).encode()).hexdigest()[:12]
        out = os.path.join(tempfile.gettempdir(), f"lfg_{name}_{os.getuid()}_{tag}.so")
        if not os.path.exists(out):
            tmp = out + f".{os.getpid()}"
            subprocess.check_call(cmd + ["-o", tmp, src, *libs])
            os.replace(tmp, out)
        L = ctypes.CDLL(out)
        for fn, argtypes in signatures.items():
            getattr(L, fn).argtypes = argtypes
            getattr(L, fn).restype = None
        _libs[key] = L
    return _libs[key]


def ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def frames_and_vectors(prev, curr, mv):
    """(prev, curr, mv) as the C loops read them: contiguous, (H, W, 4) uint8 twice and (H, W, 2) int8."""
    prev = np.ascontiguousarray(prev, np.uint8)
    curr = np.ascontiguousarray(curr, np.uint8)
    mv = np.ascontiguousarray(np.asarray(mv).astype(np.int8, copy=False))
    assert prev.shape == curr.shape and prev.shape[2] == 4 and mv.shape == prev.shape[:2] + (2,)
    return prev, curr, mv
