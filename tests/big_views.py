"""Views of 2 GiB and 4 GiB into one large device allocation: the geometry, the 32-bit aliases it is built around and the staging
that tests/test_gpu_big_views.py uses.  Plain helper: nothing here needs a GPU until `Arena` is made.

A view's rows are tens of MB apart, so a tiny image spans more than 2^31 or 2^32 bytes.  A kernel that keeps a BYTE offset in 32
bits then reads or writes another row's address without faulting.  Every view starts BASE = 2^31 bytes into an arena of ARENA =
2^31 + 2^32 + 2^28 bytes, so that each such miscalculation (aliases()) still lands inside the arena: a wrong byte, never a fault.
Offsets kept in pixels or words wrap only at 8 to 16 GiB; spans of that size are out of scope."""
from collections import namedtuple

import numpy as np

from linux_fg_amd import capi

BASE = 2 ** 31
ARENA = 2 ** 31 + 2 ** 32 + 2 ** 28
SENTINEL = 0xC3
GUARD = 64                                          # sentinel bytes checked to the right of every row of an output view
MARGIN = 2 ** 20

TALL = ("tall2", "tall2_4", "tall4", "tall4_4")
GEOMETRIES = TALL + ("pitch31",)
# what a "+4" geometry adds to the pitch: an RGBA8 or vector frame keeps its rows 4-byte aligned; a mask and a luma plane may
# have any alignment, a chroma plane 2 bytes
BUMP = {"frame": 4, "byte": 1, "uv": 2}


def pitch_of(geometry, rows, kind="frame"):
    """The pitch of a view of `rows` rows: the smallest multiple of 16 that puts the last row 2^31 (tall2) or 2^32 (tall4) plus
    MARGIN bytes behind the first, that plus BUMP for the _4 geometries, and 2^31 + 64 for pitch31 (two rows fit the arena)."""
    if geometry == "pitch31":
        return 2 ** 31 + 64
    span = (2 ** 31 if geometry.startswith("tall2") else 2 ** 32) + MARGIN
    pitch = -(-span // (rows - 1))
    pitch += -pitch % 16
    return pitch + (BUMP[kind] if geometry.endswith("_4") else 0)


def fits(geometry, rows, row_bytes, kind="frame"):
    return (rows - 1) * pitch_of(geometry, rows, kind) + row_bytes <= 2 ** 32 + 2 ** 28


def _i32(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


# name -> (the offset a 32-bit miscalculation of y * pitch + x gives, the true offsets it gets right)
ALIASES = {
    "u32(y * P + x)": (lambda y, p, x: (y * p + x) % 2 ** 32, lambda t, y, p: t < 2 ** 32),
    "i32(y * P + x)": (lambda y, p, x: _i32(y * p + x), lambda t, y, p: t < 2 ** 31),
    "y * i32(P) + x": (lambda y, p, x: y * _i32(p) + x, lambda t, y, p: p < 2 ** 31 or y == 0),
    "i32(y * P) + x": (lambda y, p, x: _i32(y * p) + x, lambda t, y, p: y * p < 2 ** 31),
    "u32(y * P) + x": (lambda y, p, x: (y * p) % 2 ** 32 + x, lambda t, y, p: y * p < 2 ** 32),
}


def aliases(geometry, rows, row_bytes, kind="frame"):
    """[(name, true offset, aliased offset, whether the two must be equal)] for the first and the last byte of every row."""
    pitch = pitch_of(geometry, rows, kind)
    out = []
    for y in range(rows):
        for x in (0, row_bytes - 1):
            t = y * pitch + x
            out += [(name, t, wrong(y, pitch, x), right(t, y, pitch)) for name, (wrong, right) in ALIASES.items()]
    return out


# ---- the calls and their operands: what tests/test_gpu_big_views.py runs, and what tests/test_big_views.py checks the aliases of

IMAGE = (64, 40)
DOWN = ((63, 39), (21, 13))                         # the 3:1 downscale
PLANE = {"rgba": "frame", "mv": "frame", "mvq": "frame", "mask": "byte", "y": "byte", "uv": "uv"}
Operand = namedtuple("Operand", "kind role rows row_bytes")


def _o(kind, role, size="same"):
    return kind, role, size


_PAIR = {"prev": _o("rgba", "in"), "curr": _o("rgba", "in")}
_MC = dict(_PAIR, mv=_o("mv", "in"))
_OUT = {"out": _o("rgba", "out")}
_OUT1, _OUT2 = {"out0": _o("rgba", "out")}, {"out0": _o("rgba", "out"), "out1": _o("rgba", "out")}

# call -> operand -> (kind, "in" or "out", size: "same", "2x", "half" or (width, height))
OPERANDS = {
    "scale_2x": {"in": _o("rgba", "in"), "out": _o("rgba", "out", "2x")},
    "scale_generic": {"in": _o("rgba", "in"), "out": _o("rgba", "out", (96, 60))},
    "motion": dict(_PAIR, mv=_o("mv", "out")),
    "interpolate_centre": dict(_MC, **_OUT1), "interpolate_random": dict(_MC, **_OUT1),
    "interpolate_multi_centre": dict(_MC, **_OUT2), "interpolate_multi_random": dict(_MC, **_OUT2),
    "interpolate_scale": dict(_MC, out=_o("rgba", "out", "2x")),
    "mv_export": {"mv": _o("mv", "in")},
    "motion_pyramid": dict(_PAIR, mv=_o("mv", "out")),
    "motion_refine": dict(_PAIR, mv_in=_o("mv", "in"), mv_out=_o("mv", "out")),
    "frame_halve": {"src": _o("rgba", "in"), "dst": _o("rgba", "out", "half")},
    "motion_expand": dict(_PAIR, mv_low=_o("mv", "in", "half"), mv_out=_o("mv", "out")),
    "motion_subpel": dict(_PAIR, mv_in=_o("mv", "in"), mvq=_o("mvq", "out")),
    "compensated": dict(_MC, **_OUT), "compensated_reach32": dict(_MC, **_OUT),
    "masked": dict(_MC, mask=_o("mask", "in"), **_OUT),
    "bidirectional": dict(_MC, bwd=_o("mv", "in"), **_OUT),
    "extrapolate": dict(_MC, **_OUT),
    "subpel": dict(_PAIR, mv=_o("mvq", "in"), **_OUT),
    "bicubic": dict(_MC, **_OUT), "bicubic_q2": dict(_PAIR, mv=_o("mvq", "in"), **_OUT),
    "static_mask": dict(_PAIR, mask=_o("mask", "out")),
    "motion_consistency": {"a": _o("mv", "in"), "b": _o("mv", "in"), "mask": _o("mask", "out")},
    "hole_fill_plane": {"keys": _o("rgba", "in"), "plane": _o("rgba", "out")},
    "pair_match": dict(_MC),
    "cut_fallback": dict(_PAIR, **_OUT2),
    "frame_diff": {"a": _o("rgba", "in"), "b": _o("rgba", "in")},
    "frame_ssim": {"a": _o("rgba", "in"), "b": _o("rgba", "in")},      # no pitch31 for planes: it has none, and 8 x 8 windows want 8 rows
    "nv12_to_rgba_left": {"y": _o("y", "in"), "uv": _o("uv", "in"), "rgba": _o("rgba", "out")},
    "nv12_to_rgba_replicate": {"y": _o("y", "in"), "uv": _o("uv", "in"), "rgba": _o("rgba", "out")},
    "rgba_to_nv12_left": {"rgba": _o("rgba", "in"), "y": _o("y", "out"), "uv": _o("uv", "out")},
    "rgba_to_nv12_replicate": {"rgba": _o("rgba", "in"), "y": _o("y", "out"), "uv": _o("uv", "out")},
    "sharpen": {"src": _o("rgba", "in"), "dst": _o("rgba", "out")},
    "resample_up": {"src": _o("rgba", "in"), "dst": _o("rgba", "out", (96, 60))},
    "resample_down": {"src": _o("rgba", "in", DOWN[0]), "dst": _o("rgba", "out", DOWN[1])},
    "resample_antiring": {"src": _o("rgba", "in"), "dst": _o("rgba", "out", (96, 60))},
    "frame_copy": {"src": _o("rgba", "in"), "dst": _o("rgba", "out")},
    "frame_upload": {"dst": _o("rgba", "out")}, "frame_download": {"src": _o("rgba", "in")},
    "ring_upload": {"dst": _o("rgba", "out")}, "ring_download": {"src": _o("rgba", "in")},
}
for _s in ("default", "fused", "pyramid_compensated"):
    OPERANDS[f"frames_{_s}"] = dict(_PAIR, **_OUT1)
    OPERANDS[f"frames_multi_{_s}"] = dict(_PAIR, **_OUT2)

# The pitch31 geometry for masks and planes: the image at which the big plane has two rows.  Every call with a mask or a plane
# runs at two rows; lfg_frame_ssim, the one call that needs more rows than that, has no mask or plane operand.
PITCH31_IMAGE = {"mask": (64, 2), "y": (64, 2), "uv": (64, 4)}


def operands_of(name, w, h):
    """operand -> Operand(kind, role, rows, row bytes) of the call at an image of w x h."""
    out = {}
    for op, (kind, role, size) in OPERANDS[name].items():
        ow, oh = {"same": (w, h), "2x": (2 * w, 2 * h), "half": ((w + 1) // 2, (h + 1) // 2)}.get(size, size)
        rows, row_bytes = {"rgba": (oh, 4 * ow), "mv": (oh, 2 * ow), "mvq": (oh, 4 * ow), "mask": (oh, ow), "y": (oh, ow), "uv": (oh // 2, ow)}[kind]
        out[op] = Operand(kind, role, rows, row_bytes)
    return out


def tall_cases():
    """(call, big operand, geometry): every operand of every call in turn at the four tall geometries."""
    return [(name, op, g) for name in OPERANDS for op in OPERANDS[name] for g in TALL]


def frame_operands():
    """(call, operand) for every lfg_frame operand: the refusals of pitch31."""
    return [(name, op) for name in OPERANDS for op, (kind, _, _) in OPERANDS[name].items() if PLANE[kind] == "frame"]


def plane_cases():
    """(call, operand, width, height) for every mask and plane operand: pitch31 at two rows."""
    return [(name, op) + PITCH31_IMAGE[kind] for name in OPERANDS for op, (kind, _, _) in OPERANDS[name].items() if PLANE[kind] != "frame"]


# ---- the arena and the staging (GPU)

def _bytes(ctx, address, count):
    """`count` (even) bytes at a device address as a one-row tight frame."""
    assert count % 2 == 0
    return capi.Context.wrap(address, count // 2, 1, capi.FORMAT_MV_S8X2, pitch=count)


def write_rows(ctx, address, pitch, rows2d, right=0, fill=SENTINEL):
    """rows2d (rows, n) uint8 into rows `pitch` apart, each followed by `right` bytes of `fill`: one tight one-row upload per
    row, which depends on no pitch handling of the library."""
    rows, n = rows2d.shape
    count = n + right + (n + right) % 2
    line = np.full(count, fill, np.uint8)
    for y in range(rows):
        line[:n] = rows2d[y]
        ctx.upload(_bytes(ctx, address + y * pitch, count), line.view(np.int8).reshape(1, -1, 2))


def read_rows(ctx, address, pitch, rows, n, right=0):
    """((rows, n) uint8, (rows, right) uint8): the rows and the bytes to their right."""
    count = n + right + (n + right) % 2
    got = np.stack([ctx.download(_bytes(ctx, address + y * pitch, count)).view(np.uint8).reshape(-1) for y in range(rows)])
    return got[:, :n], got[:, n:n + right]


def hip_runtime():
    """The HIP runtime that liblinuxfg_hip.so itself runs on, found among the process's mappings.  torch's wheel brings a runtime of
    its own under the same name: where torch was imported first the library is bound to that one, and it is the only one mapped;
    where the library was loaded first, torch's is a second runtime, which finds no GPU in a process that has a context.  So a
    torch tensor cannot be the arena in every order of the suite, and the allocation goes to the runtime the library uses."""
    import ctypes
    import os
    capi.load()
    with open("/proc/self/maps") as maps:
        paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    own = paths if len(paths) == 1 else [p for p in paths if os.sep + "torch" + os.sep not in p]
    assert len(own) == 1, f"which HIP runtime does the library use: {paths}"
    return ctypes.CDLL(own[0])


class Arena:
    """One device allocation of ARENA bytes (lfg_frame_create stops at 32768 x 32768), made with the library's own HIP runtime
    on the device of the context.  `free` is what the device had left before it was made."""

    def __init__(self, ctx):
        import ctypes
        self.hip = hip_runtime()
        assert self.hip.hipSetDevice(int(ctx.lib.lfg_context_device(ctx.h))) == 0
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert self.hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        self.free, self.base = free.value, None
        if self.free < ARENA + 2 ** 30:
            return
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(ARENA)) == 0, "hipMalloc of the arena"
        self.base = p.value
        assert self.base % 256 == 0
        self.view = self.base + BASE                # where every big view starts

    def release(self):
        import ctypes
        if self.base:
            assert self.hip.hipFree(ctypes.c_void_p(self.base)) == 0
        self.base = None
