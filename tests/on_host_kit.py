"""What the *_on_host tests that go through tests/cpp/hip_on_host share: the three builds of a driver program (g++ alone, the
csrc/*.hip files compiled as C++ with the stand-in <hip/hip_runtime.h> in front of every other include directory), the probe
that skips a sanitized build where g++ has no runtime for it, the three frame layouts, and one run of a driver over a list of
cases.  The sanitized code is always the stand-alone program; nothing here is loaded into Python."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
# Where the kernels and the layer are taken from.  The two variables exist for one purpose: to show that a planted fault -- a
# guard off by one in a copy of csrc, a per-lane ballot in a copy of the layer -- fails these tests.
# Such a copy lies outside the repository, and every build under an override says so on stderr: a stale variable cannot make
# the suite test another tree unnoticed.
DEFAULT_CSRC, DEFAULT_LAYER = os.path.join(ROOT, "linux-fg_amd", "csrc"), os.path.join(CPP, "hip_on_host")
CSRC = os.environ.get("LFG_ON_HOST_CSRC", DEFAULT_CSRC)
LAYER = os.environ.get("LFG_ON_HOST_LAYER", DEFAULT_LAYER)
# The address-sanitized build is not optimised: the kernels load from a clamped address and select afterwards (texel_or_zero),
# and from -O1 on g++ sinks such a load into the branch that uses it, so the access the device makes would never happen here.
FLAGS = {"plain": ["-O1"], "sanitized": ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
         "thread": ["-O1", "-g", "-fsanitize=thread"]}
# -ffp-contract=off: as csrc/Makefile has it.  The pragmas are hipcc's (#pragma unroll).
COMMON = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
          "-pthread", "-I", LAYER, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", CPP]
SENTINEL = 0x5A


def build(tmp_path_factory, kind, name, hip_files):
    """tests/cpp/<name>.cpp and the csrc files `hip_files`, each its own translation unit, as the program <name> of build `kind`
    (plain / sanitized / thread).  Skips where g++ has no runtime for the build's sanitizer."""
    for variable, used, default in (("LFG_ON_HOST_CSRC", CSRC, DEFAULT_CSRC), ("LFG_ON_HOST_LAYER", LAYER, DEFAULT_LAYER)):
        if os.path.realpath(used) != os.path.realpath(default):
            inside = os.path.commonpath([os.path.realpath(used), os.path.realpath(ROOT)]) == os.path.realpath(ROOT)
            assert not inside, f"{variable}={used} lies inside the repository: an override is a copy elsewhere"
            print(f"on_host_kit: {name} ({kind}) is built from {variable}={used}, NOT from the repository", file=sys.stderr)
    out = tmp_path_factory.mktemp(f"{name}_{kind}")
    sanitize = [f for f in FLAGS[kind] if f.startswith("-fsanitize=")]
    if sanitize:
        probe = out / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++", *sanitize, str(probe), "-o", str(out / "probe")], capture_output=True).returncode != 0:
            pytest.skip("this g++ has no runtime for " + " ".join(sanitize))
    units = [(os.path.join(CPP, name + ".cpp"), out / (name + ".o"))] + [(os.path.join(CSRC, f), out / (f + ".o")) for f in hip_files]

    def compile_one(unit):
        p = subprocess.run(["g++", *FLAGS[kind], *COMMON, "-x", "c++", "-c", unit[0], "-o", str(unit[1])], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]

    with ThreadPoolExecutor(max_workers=4) as pool:
        list(pool.map(compile_one, units))
    subprocess.check_call(["g++", *FLAGS[kind], "-pthread", *[str(o) for _, o in units], "-o", str(out / name)])
    return out / name


# ---- frames that end where they end.  A layout is (lead, pad): `lead` bytes in front of the first row and `pad` bytes after
# every row but the last, so the allocation is lead + (H - 1) * pitch + W * bpp bytes.  "poisoned": lead and pitch are
# multiples of 8 and the driver poisons lead and padding (ASan's granules are 8 bytes; a row may still end inside one);
# "sentinel": a pitch that is only 4-byte aligned (2-byte for vectors, 1 for masks), lead and padding hold 0x5A.
LAYOUTS = ("tight", "poisoned", "sentinel")
# "poisoned16": "poisoned" with lead and pitch multiples of 16, for the record kernels, which take a 16-byte walk where base
# and pitch allow.
RECORD_LAYOUTS = LAYOUTS + ("poisoned16",)


def layout(kind, width_bytes, unit):
    """(lead, pitch, poison) of a buffer with rows of `width_bytes` whose pitch must be a multiple of `unit` bytes."""
    if kind == "tight":
        return 0, width_bytes, 0
    if kind == "poisoned":
        return 16, (width_bytes + 8 + 7) // 8 * 8, 1
    if kind == "poisoned16":
        return 16, (width_bytes + 16 + 15) // 16 * 16, 1
    return 2 * unit, width_bytes + 3 * unit, 0


class Cases:
    """The cases of one run of a driver: `add` writes the input buffers of a case (rows only, the driver lays them out) and one
    line of the driver's manifest; `run` runs the driver once over all of them and returns each case's outputs."""

    def __init__(self, directory):
        self.dir = directory
        self.lines = []
        self.outputs = []
        self.n = 0

    def buffer(self, array, kind, unit):
        """An input: "path:lead:pitch:poison"."""
        array = np.ascontiguousarray(array)
        h = array.shape[0]
        width_bytes = array.nbytes // h
        path = os.path.join(self.dir, f"in{self.n}.bin")
        self.n += 1
        array.tofile(path)
        lead, pitch, poison = layout(kind, width_bytes, unit)
        return f"{path}:{lead}:{pitch}:{poison}"

    def output(self, shape, dtype, kind, unit):
        """An output: "path:lead:pitch:poison"; the driver writes the whole allocation, lead and padding included."""
        h = shape[0]
        width_bytes = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
        path = os.path.join(self.dir, f"out{self.n}.bin")
        self.n += 1
        lead, pitch, poison = layout(kind, width_bytes, unit)
        return f"{path}:{lead}:{pitch}:{poison}", (path, shape, np.dtype(dtype), lead, pitch, width_bytes, poison)

    def add(self, words, outputs, label):
        self.lines.append(" ".join(str(w) for w in words))
        self.outputs.append((label, outputs))

    def run(self, program, env=None):
        manifest = os.path.join(self.dir, "manifest.txt")
        with open(manifest, "w") as f:
            f.write("\n".join(self.lines) + "\n")
        p = subprocess.run([str(program), manifest], capture_output=True, text=True, env=env)
        assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-6000:])
        assert p.stdout.strip().endswith(f"ok {len(self.lines)}"), p.stdout[-1500:]
        results = []
        for label, outputs in self.outputs:
            arrays = []
            for path, shape, dtype, lead, pitch, width_bytes, poison in outputs:
                raw = np.fromfile(path, np.uint8)
                h = shape[0]
                assert raw.size == lead + (h - 1) * pitch + width_bytes, (label, raw.size)
                assert (raw[:lead] == SENTINEL).all(), f"{label}: the bytes in front of the first row were written"
                rows = np.empty((h, width_bytes), np.uint8)
                for y in range(h):
                    rows[y] = raw[lead + y * pitch: lead + y * pitch + width_bytes]
                    if y + 1 < h:
                        assert (raw[lead + y * pitch + width_bytes: lead + (y + 1) * pitch] == SENTINEL).all(), f"{label}: row {y}'s padding was written"
                arrays.append(rows.view(dtype).reshape(shape))
            results.append(arrays)
        return results


# ---- what the drivers' tests share of their cases

END_BYTES = np.array([127, 128, 129, 0, 1, 255, 64, 192], np.uint8)


def end_fields(w, h, seed):
    """Vector fields that put the ends of MV_S8X2's range at every border and corner: every component -128, -127 or 127; the same
    for one uniform vector per sign pattern; and every byte one of 127, 128, 129, 0, 1, 255, 64, 192."""
    rng = np.random.default_rng(seed)
    yield "ends", rng.choice(np.array([-128, -127, 127], np.int8), (h, w, 2))
    for k, v in enumerate(((127, 127), (-128, -128), (-127, 127), (127, -128))):
        if (seed + k) % 4 == 0:                       # one uniform field per size, all four over the sizes
            f = np.empty((h, w, 2), np.int8)
            f[...] = v
            yield f"uniform{v}", f
    yield "bytes", rng.choice(END_BYTES, (h, w, 2)).view(np.int8)


def end_fields_q(w, h, seed):
    """The same for MV_S16X2_Q2, which accepts every 16-bit value and clamps to +-508."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-32768, 32767, -509, -508, 508, 509, -505, 507], np.int16), (h, w, 2))


def f32(t):
    return "%.9g" % np.float32(t)


def sweep(sizes):
    """(k, w, h, layout): every size under every layout, k counting on so that parameters can rotate through their lists."""
    k = 0
    for w, h in sizes:
        for lay in LAYOUTS:
            yield k, w, h, lay
            k += 1


def first_bad(got, want):
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(-1))
    y, x = bad[0]
    return f"{len(bad)} differ, first at x={x} y={y}: got {got[y, x]} want {want[y, x]}"
