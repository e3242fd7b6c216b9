"""What the CPU models with C loops share (pyramid_model.py, refine_model.py and the compensated family: mc_model.py,
overlay_model.py, extrapolate_model.py, bidir_model.py): the loader of their C sources, built with the system C compiler on
first use, the hand-over of numpy arrays to them, and what the family's four wrappers have in common, as
tests/compensated_model.h holds what their C sources have in common."""
from __future__ import annotations

import ctypes
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = re.compile(rb'^[ \t]*#[ \t]*include[ \t]*"([^"\n]+)"', re.M)
_libs = {}

VP, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float       # for the models' signatures
HOLE = 0xFFFFFFFF                                              # the compensated family's key image: nothing landed here
DEFAULT_MATCH_SAD = 48


def build_tag(src, command) -> str:
    """The cache tag of one build: a hash of the command's words and of every file the compiler reads, which is `src` and each
    #include "..." it names, resolved next to the file that names it and followed through the headers' own includes."""
    files, todo = [], [os.path.abspath(src)]
    while todo:
        path = todo.pop()
        if path not in files:
            files.append(path)
            todo += [os.path.normpath(os.path.join(os.path.dirname(path), inc.decode()))
                     for inc in _INCLUDE.findall(open(path, "rb").read())]
    h = hashlib.sha1(" ".join(command).encode())
    for path in sorted(files):
        h.update(b"\0" + open(path, "rb").read())
    return h.hexdigest()[:12]


def load(name, signatures, flags=(), libs=()):
    """tests/<name>.c as a ctypes library, built with cc -O2 -shared -fPIC `flags` ... `libs`.  `signatures` gives the argtypes
    of its functions (all return void).  The build is cached in the temp directory under a name made from build_tag, so an
    edited source, an edited header or another set of flags never loads a stale library; the rename makes a half-written file
    invisible to a test process running next to this one."""
    key = (name, tuple(flags), tuple(libs))
    if key not in _libs:
        src = os.path.join(_HERE, name + ".c")
        cmd = [os.environ.get("CC", "cc"), "-O2", "-shared", "-fPIC", *flags]
        out = os.path.join(tempfile.gettempdir(), f"lfg_{name}_{os.getuid()}_{build_tag(src, cmd + list(libs))}.so")
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


def mutant_loader(name, signatures, macro_prefix, mutants):
    """load_(mutant=None): tests/<name>.c with -ffp-contract=off, or with mutant = one of `mutants` the same source built with
    -D<macro_prefix><mutant>, under a cache name of its own."""
    def load_(mutant=None):
        assert mutant is None or mutant in mutants, mutant
        return load(name, signatures, ["-ffp-contract=off"] + ([f"-D{macro_prefix}{mutant}"] if mutant else []), ["-lm"])
    return load_


def ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def plane(a, dtype, shape):
    """`a` as the C loops read it: contiguous, of `dtype` and of exactly `shape`."""
    a = np.ascontiguousarray(np.asarray(a).astype(dtype, copy=False))
    assert a.shape == tuple(shape), (a.shape, shape)
    return a


def frames_and_vectors(prev, curr, mv):
    """(prev, curr, mv) as the C loops read them: contiguous, (H, W, 4) uint8 twice and (H, W, 2) int8."""
    prev = np.ascontiguousarray(prev, np.uint8)
    assert prev.ndim == 3 and prev.shape[2] == 4, prev.shape
    return prev, plane(curr, np.uint8, prev.shape), plane(mv, np.int8, prev.shape[:2] + (2,))


def key(vx: int, vy: int) -> int:
    """A vector's projection key: the smallest key wins (longest vector, then smallest vy, then smallest vx)."""
    return ((65535 - (vx * vx + vy * vy)) << 16) | ((vy + 128) << 8) | (vx + 128)


def sampling(K, H, W, roi):
    """What every sample() of the family starts from: the key image as the C loops read it, the rectangle
    (x0, y0, x1, y1) of roi = (x, y, w, h) or of the whole frame, and the (h, w, 4) uint8 array to fill."""
    x, y, w, h = roi if roi is not None else (0, 0, W, H)
    return plane(K, np.uint32, (H, W)), (x, y, x + w, y + h), np.empty((h, w, 4), np.uint8)
