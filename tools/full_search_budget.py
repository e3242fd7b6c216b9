#!/usr/bin/env python3
"""Static instruction budget of the two full-search phases of the persistent motion kernel: what ONE pass of the narrow
search (prefilter_narrow.inc) and of the row band (prefilter_rowband.inc) issues, by kind of instruction.  No GPU needed.

    tools/full_search_budget.py                      compile csrc/motion_prefilter.hip to assembly (the Makefile's flags plus
                                                     --cuda-device-only -S) and print the table for motion_prefilter_kernel<false, 0>
    tools/full_search_budget.py --asm FILE.s         the same for an assembly file made earlier (another commit's, say)
    tools/full_search_budget.py --kernel ILb0ELi1E   another instantiation (a substring of the mangled name)

How the loops are found.  The record paths carry the markers `; some lane records a candidate (narrow)` / `(row band)`.
The innermost loop around a phase's markers is its loop over the candidates of a pass (the test, one copy, `nounroll`); the
loop around that one is the per-pass loop.  The compiler's own loop comments on the basic blocks give the nesting.  The
per-pass loop is then cut, in layout order, into
    head      from the loop's first block to the candidate loop     (bookkeeping, order entry, window reads; for the row band
                                                                     also the slab reads, the row sums and the test of both candidates)
    no-hit    the cheapest way once round the candidate loop that    (per candidate; what a candidate that no lane records costs.
              reads the slab                                          The row band tests a pass's two candidates at once, in the
                                                                     head: its candidate loop is hit side altogether)
    hit side  the rest of the candidate loop                         (static size only: not on the path of most candidates)
    compute   from the candidate loop to the last LDS write          (distances, column sums, slab write)
    tail      what is left                                           (loop bookkeeping)
Instructions are classified by the prefix of the mnemonic alone -- v_ (VALU), s_ (scalar), ds_ (LDS), global_ / flat_ /
scratch_ / buffer_ (memory) -- except the lane moves v_readlane / v_writelane (scalar spills and reloads), counted apart.
These are static counts: a block counts once however often its branch is taken."""
from __future__ import annotations

import argparse
import heapq
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linux-fg_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
         "-fvisibility=hidden", f"-I{os.path.join(ROOT, 'include')}", "-Wall", "-Wno-unused-function"]
KINDS = ("valu", "scalar", "lds", "memory", "lane moves")
MARKERS = {"narrow search": "; some lane records a candidate (narrow)", "row band": "; some lane records a candidate (row band)"}


def classify(mnemonic: str) -> str | None:
    if mnemonic.startswith(("v_readlane", "v_writelane")):
        return "lane moves"
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("s_"):
        return "scalar"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "memory"
    return None


class Block:
    def __init__(self, name: str, index: int):
        self.name, self.index = name, index
        self.header = None           # innermost loop header (a block name), None outside every loop
        self.is_header = False
        self.parents: list[str] = []  # enclosing headers, outermost first (known for header blocks only)
        self.insts: list[str] = []    # mnemonics
        self.operands: list[str] = []
        self.markers: set[str] = set()
        self.last_lds_write = -1      # index into insts

    def counts(self, upto: int | None = None, frm: int = 0) -> dict[str, int]:
        c = dict.fromkeys(KINDS, 0)
        for m in self.insts[frm:upto]:
            k = classify(m)
            if k:
                c[k] += 1
        return c


def parse_kernel(lines: list[str], kernel: str) -> list[Block]:
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(kernel) + r"\w*:", l)), None)
    if start is None:
        sys.exit(f"no kernel matching {kernel!r} in the assembly")
    blocks = [Block("entry", 0)]
    for line in lines[start + 1:]:
        if line.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):|^; (%bb\.\d+):", line)
        if m:
            blocks.append(Block(m.group(1) or m.group(2), len(blocks)))
        b = blocks[-1]
        note = line.split(";", 1)[1] if ";" in line else ""
        if (h := re.search(r"in Loop: Header=(BB\d+_\d+)", note)):
            b.header = ".L" + h.group(1)
        if (p := re.search(r"Parent Loop (BB\d+_\d+)", note)):
            b.parents.append(".L" + p.group(1))
        if re.search(r"This (Inner )?Loop Header", note):
            b.is_header, b.header = True, b.name
        for phase, text in MARKERS.items():
            if text in line:
                b.markers.add(phase)
        body = line.split(";", 1)[0].strip()
        if not body or body.startswith(".") or body.endswith(":"):
            continue
        parts = body.split(None, 1)
        b.insts.append(parts[0])
        b.operands.append(parts[1] if len(parts) > 1 else "")
        if parts[0].startswith("ds_write"):
            b.last_lds_write = len(b.insts) - 1
    return blocks


def loop_of(blocks: list[Block], header: str) -> list[Block]:
    """Every block of the loop with that header, inner loops included, in layout order."""
    parent = {b.name: (b.parents[-1] if b.parents else None) for b in blocks if b.is_header}
    def inside(h):
        while h is not None:
            if h == header:
                return True
            h = parent.get(h)
        return False
    return [b for b in blocks if inside(b.header)]


def cheapest_cycle(blocks: list[Block], loop: list[Block], header: str) -> list[Block]:
    """The cheapest path (in instructions) from the loop's header back to it that reads LDS on its way -- the slab reads of a
    candidate; a way round the loop that tests nothing (the loop's own exit check) does not count.  Empty if there is none."""
    by_name = {b.name: b for b in blocks}
    members = {b.name for b in loop}
    def successors(b: Block):
        out, falls = [], True
        for m, o in zip(b.insts, b.operands):
            if m.startswith("s_cbranch") or m == "s_branch":
                out.append(o.strip())
                falls = m != "s_branch"
        if falls and b.index + 1 < len(blocks):
            out.append(blocks[b.index + 1].name)
        return out
    def reads_lds(b: Block) -> bool:
        return any(m.startswith("ds_") for m in b.insts)
    first = (header, reads_lds(by_name[header]))
    best = {first: (len(by_name[header].insts), [header])}
    heap = [(len(by_name[header].insts), first)]
    while heap:
        cost, state = heapq.heappop(heap)
        if cost > best[state][0]:
            continue
        name, seen = state
        for s in successors(by_name[name]):
            if s == header:
                if seen:
                    return [by_name[n] for n in best[state][1]]
                continue
            if s not in members:
                continue
            nxt, c = (s, seen or reads_lds(by_name[s])), cost + len(by_name[s].insts)
            if nxt not in best or c < best[nxt][0]:
                best[nxt] = (c, best[state][1] + [s])
                heapq.heappush(heap, (c, nxt))
    return []


def add(total: dict[str, int], c: dict[str, int]) -> None:
    for k in KINDS:
        total[k] += c[k]


def budget(blocks: list[Block], phase: str) -> dict[str, dict[str, int]]:
    marked = [b for b in blocks if phase in b.markers]
    if not marked:
        sys.exit(f"no record marker of the {phase} in this kernel")
    cand_header = marked[0].header
    headers = {b.name: b for b in blocks if b.is_header}
    pass_header = headers[cand_header].parents[-1]
    pass_loop, cand_loop = loop_of(blocks, pass_header), loop_of(blocks, cand_header)
    cand_names = {b.name for b in cand_loop}
    first_cand, last_cand = cand_loop[0].index, cand_loop[-1].index
    no_hit = cheapest_cycle(blocks, cand_loop, cand_header)
    no_hit_names = {b.name for b in no_hit}
    after = [b for b in pass_loop if b.index > last_cand and b.name not in cand_names]
    last_write = max((b.index for b in after if b.last_lds_write >= 0), default=-1)
    parts = {p: dict.fromkeys(KINDS, 0) for p in ("head", "no-hit path, per candidate", "hit side (static)", "compute side", "tail")}
    for b in pass_loop:
        if b.name in cand_names:
            add(parts["no-hit path, per candidate" if b.name in no_hit_names else "hit side (static)"], b.counts())
        elif b.index < first_cand:
            add(parts["head"], b.counts())
        elif b.index < last_write:
            add(parts["compute side"], b.counts())
        elif b.index == last_write:
            add(parts["compute side"], b.counts(upto=b.last_lds_write + 1))
            add(parts["tail"], b.counts(frm=b.last_lds_write + 1))
        else:
            add(parts["tail"], b.counts())
    return parts


def report(blocks: list[Block], out) -> None:
    whole = dict.fromkeys(KINDS, 0)
    for b in blocks:
        add(whole, b.counts())
    print("whole kernel: " + ", ".join(f"{whole[k]} {k}" for k in KINDS), file=out)
    for phase in MARKERS:
        parts = budget(blocks, phase)
        print(f"\nper-pass loop of the {phase}", file=out)
        print(f"  {'part':28s}" + "".join(f"{k:>11s}" for k in KINDS) + f"{'all':>8s}", file=out)
        for name, c in parts.items():
            print(f"  {name:28s}" + "".join(f"{c[k]:11d}" for k in KINDS) + f"{sum(c.values()):8d}", file=out)
        once = [p for p in parts if p not in ("no-hit path, per candidate", "hit side (static)")]
        fixed = sum(sum(parts[p].values()) for p in once)
        per = sum(parts["no-hit path, per candidate"].values())
        print(f"  a pass nobody records in: {fixed} + {per} per candidate tested one after the other", file=out)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--asm", help="an assembly file made earlier, instead of compiling")
    ap.add_argument("--kernel", default="motion_prefilter_kernelILb0ELi0E", help="substring of the kernel's mangled name")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "motion_prefilter.s")
            subprocess.check_call([args.hipcc, *FLAGS, "--cuda-device-only", "-S", "motion_prefilter.hip", "-o", s],
                                  cwd=CSRC, stderr=subprocess.DEVNULL)
            text = open(s).read()
    report(parse_kernel(text.split("\n"), args.kernel), sys.stdout)


if __name__ == "__main__":
    main()
