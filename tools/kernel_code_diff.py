#!/usr/bin/env python3
"""Compare the machine code of named kernels between two builds of liblinuxfg_hip.so.

    python tools/kernel_code_diff.py OLD.so NEW.so mc_interpolate_kernel bidir_sample_kernel ...

Each library's gfx950 code objects are extracted with `llvm-objdump --offloading` and disassembled; for every symbol whose
name contains one of the given names, the instruction words (the hex column of the disassembly, so neither addresses nor the
numbering of labels take part) are compared.  Prints one line per symbol and exits 1 if any differs or is missing on either
side.  A name matches its mangled symbol and nothing longer: `mc_interpolate_kernel` does not match
`mc_interpolate_masked_kernel`, because the mangled name carries the length."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "linux-fg_amd", "csrc"))
from check_store_hazard import OBJDUMP      # the ROCm toolchain's llvm-objdump, found as the build's own check finds it

_SYMBOL = re.compile(r"^[0-9a-f]+ <(\S+)>:$")
_WORDS = re.compile(r"//\s*[0-9A-Fa-f]+:\s*((?:[0-9A-Fa-f]{8}\s*)+)$")


def kernels(lib):
    """{symbol: [instruction words]} over every code object bundled in `lib`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.run([OBJDUMP, "--offloading", local], check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            text = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            name = None
            for line in text.splitlines():
                m = _SYMBOL.match(line)
                if m:
                    name = m.group(1)
                    out[name] = []
                    continue
                w = _WORDS.search(line)
                if w and name:
                    out[name] += w.group(1).split()
    return out


def main():
    old, new, names = kernels(sys.argv[1]), kernels(sys.argv[2]), sys.argv[3:]
    bad = 0
    for n in names:
        tag = f"{len(n)}{n}"                  # the Itanium mangling's <length><name>
        symbols = sorted(s for s in set(old) | set(new) if tag in s and not s.endswith(".kd"))
        if not symbols:
            print(f"{n}: no such symbol in either library")
            bad += 1
        for s in symbols:
            a, b = old.get(s), new.get(s)
            same = a is not None and a == b and len(a) > 0
            bad += not same
            print(f"{s}: " + (f"identical, {len(a)} words" if same else
                              "missing on one side" if a is None or b is None else f"DIFFERENT ({len(a)} against {len(b)} words)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
