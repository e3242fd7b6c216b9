"""Frame pairs and knob rows for the launch-geometry tests (tests/test_gpu_launch_geometry.py, tests/test_gpu_comm_geometry.py),
CPU side only: nothing here touches a GPU, tests/test_geometry_cases.py holds it to what it claims.

The persistent prefilter kernel (csrc/motion_prefilter.hip) is the one place where workgroups wait for each other, so what a
workgroup does depends on how many the launch has.  LFG_PREF_GROUPS, LFG_RESOLVE_GROUPS and LFG_DYN_PARTS_RT -- read when a
context is created -- set the grids directly; a ROW here is the environment of one fresh capi.Context.

Sizes, against the prefilter's 56 x 64 tile, the 16-row segment and the 64 x 64 minimum for hints:
    113 x 129    3 x 3 tiles, ragged on both axes
    300 x 200    tiles shared between rim and interior
    616 x 448    exactly 11 x 7 whole tiles; 308 segments, 1,232 rows of work for the resolve kernel
    1284 x 726   the lean kernel's ragged size (test_lean_kernel_on_ragged_sizes), for lean rows only
and one more, which the first GPU run of these tests showed to be needed:
    940 x 1000   17 x 16 tiles, ragged.  prefilter_plan shares EVERY tile of a frame between several units while the frame has
                 fewer tiles than half the slots (512 on 256 CUs: below 257 tiles), and only a unit that holds a whole tile hands a
                 segment over -- at the three sizes above the run-time queue stays empty whatever the content, and a workgroup
                 never comes to own a slot.  272 tiles is the smallest frame of this shape whose interior tiles are whole.
"""
import functools

import numpy as np

from linux_fg_amd import synth
from tests.test_gpu_parity import _lean_cases, _mixed_pair, _strip_pairs

SIZES = ((113, 129), (300, 200), (616, 448))
ORACLE_SIZES = SIZES[:2]                 # small enough for the CPU oracle on every pixel
LEAN_SIZE = (1284, 726)
HAND_OVER_SIZE = (616, 448)              # (below it the islands overlap too much for the pair to mean anything)
QUEUE_SIZE = (940, 1000)                 # whole tiles for 512 slots: the run-time queue is in use (lfg_motion_hand_over_stats)
ALL_SIZES = SIZES + (QUEUE_SIZE,)
QUEUE_MIXED_SEED = 9117

# _mixed_pair seeds: at every size in SIZES the three between them hold sensor noise, an occlusion, a static flat area and a
# fade (test_geometry_cases.py asserts it from the pixels).
MIXED_SEEDS = (9103, 9117, 9126)
INGREDIENTS = ("sensor noise", "occlusion", "static flat area", "fade")

SMALL_GRIDS = (1, 3, 8, 37)              # values coprime to the 8 XCDs among them; every workgroup takes several units
COMM_CUS = (8, 16, 24, 32)               # what LFG_COMM_CUS accepts besides 0
RESOLVE_GROUPS = (1, 5, 64)
DYN_PARTS = (4, 8)
TILE_W, TILE_H, SEGMENT_ROWS, HINT_GRID, BLOCK = 56, 64, 16, 16, 8


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def mixed_pair(size, seed):
    return _frozen(*_mixed_pair(size[0], size[1], seed))


@functools.lru_cache(maxsize=None)
def noise_pair(size):
    """Uncorrelated noise: every segment searches in full."""
    return _frozen(*synth.make_uncorrelated_pair(size[0], size[1], stream=size[0]))


def hint_sample_origins(w, h):
    """Origins of the hint kernel's 16 x 16 sample blocks of 8 x 8 texels (csrc/motion_order.hip, motion_hint_kernel)."""
    return [((2 * gx + 1) * w // (2 * HINT_GRID) - BLOCK // 2, (2 * gy + 1) * h // (2 * HINT_GRID) - BLOCK // 2)
            for gy in range(HINT_GRID) for gx in range(HINT_GRID)]


HAND_OVER_SHIFT = (5, 3)
HAND_OVER_MARGIN = 4                     # island = the sample block and 4 texels around it, 16 x 16


@functools.lru_cache(maxsize=None)
def hand_over_pair(size=HAND_OVER_SIZE):
    """test_motion_hand_over_queue_overflows_gracefully's recipe, scaled down: curr is fresh noise except islands of the panned
    prev around the hint kernel's sample blocks.  The hints say "pan" while nearly every segment finds no match once the hints
    have been tried and asks to be handed over: four times what the queue holds."""
    w, h = size
    seed = synth.BASE_SEED + 9
    prev = synth.make_prev(w, h, seed=seed)
    curr = synth.noise_bytes(w, h, 777)
    moved = synth.translate(prev, HAND_OVER_SHIFT, seed)
    m = HAND_OVER_MARGIN
    for bx, by in hint_sample_origins(w, h):
        curr[by - m:by + BLOCK + m, bx - m:bx + BLOCK + m] = moved[by - m:by + BLOCK + m, bx - m:bx + BLOCK + m]
    return _frozen(prev, curr, moved)[:2]


SCATTERED_SHIFT = (4, -3)
SCATTERED_TILES = tuple((tx, ty) for ty in (1, 2, 4, 5, 7, 8, 10, 11, 13) for tx in (2, 4, 6, 8, 10, 12))


def scattered_patches():
    """(x0, y0, width, height) of the 54 patches of scattered_pair: one inside a segment of each of SCATTERED_TILES, placed so
    that every pixel whose 8 x 8 block touches the patch lies in that one segment (segment ty % 4 of the tile)."""
    return [(TILE_W * tx + 20, TILE_H * ty + SEGMENT_ROWS * (ty % 4) + 4, 16, 8) for tx, ty in SCATTERED_TILES]


@functools.lru_cache(maxsize=None)
def scattered_pair(size=QUEUE_SIZE):
    """A pan with 54 small patches of fresh noise spread over the interior, top to bottom: 54 segments in 54 whole tiles find no
    match and are handed over one by one over the whole launch -- fewer than the queue holds, so every one goes through it --
    while every other unit ends in microseconds.  The workgroups that run out of plan units each take the next queue slot, most of
    them before anything has been pushed into it: they OWN an empty slot and poll until it is filled or the last plan unit is
    counted, which is the waiting that motion_prefilter_kernel does at all.  (With LFG_QUEUE_FIRST false, as shipped, a workgroup
    takes a slot only when the plan has no unit left for it; the branch that keeps an owned slot through a further plan unit is
    compiled out.)"""
    w, h = size
    seed = synth.BASE_SEED + 54
    prev = synth.make_prev(w, h, seed=seed)
    curr = synth.translate(prev, SCATTERED_SHIFT, seed)
    fresh = synth.noise_bytes(w, h, 5454)
    for x0, y0, pw, ph in scattered_patches():
        curr[y0:y0 + ph, x0:x0 + pw] = fresh[y0:y0 + ph, x0:x0 + pw]
    return _frozen(prev, curr)


@functools.lru_cache(maxsize=None)
def lean_pairs():
    """_lean_cases' pan and its mixture of everything, their top-left 1284 x 726: a width that is no multiple of 56, a height that
    is a multiple of neither 64 nor 16."""
    w, h = LEAN_SIZE
    wanted = ("pan", "everything the prefilter treats differently")
    out = {}
    for name, prev, curr in _lean_cases():
        if name in wanted:
            out[name] = _frozen(np.ascontiguousarray(prev[:h, :w]), np.ascontiguousarray(curr[:h, :w]))
        if len(out) == len(wanted):
            break
    return out


@functools.lru_cache(maxsize=None)
def strip_pair():
    """_strip_pairs' first case: a pan by (6, -4) at 700 x 420, which exposes a left and a bottom strip."""
    name, prev, curr, shift = next(iter(_strip_pairs()))
    return (name, *_frozen(prev, curr), shift)


def pairs_of(size):
    """{name: (prev, curr, semantics to run)} for a size in ALL_SIZES; the mixed pairs run under both tie orders."""
    if size == QUEUE_SIZE:
        return {f"mixed {QUEUE_MIXED_SEED}": (*mixed_pair(size, QUEUE_MIXED_SEED), ("reference", "intended")),
                "hand-over": (*hand_over_pair(size), ("reference",)), "scattered": (*scattered_pair(size), ("reference",))}
    out = {f"mixed {seed}": (*mixed_pair(size, seed), ("reference", "intended")) for seed in MIXED_SEEDS}
    out["noise"] = (*noise_pair(size), ("reference",))
    if size == HAND_OVER_SIZE:
        out["hand-over"] = (*hand_over_pair(size), ("reference",))
    return out


def tiles_of(size):
    return -(-size[0] // TILE_W) * -(-size[1] // TILE_H)


# ------------------------------------------------------------------ what a pair holds, read from its pixels

def _pan_of(clean_prev, curr):
    """The translation most of curr's middle is clean_prev under (|component| <= 12, as _mixed_pair draws it)."""
    h, w = curr.shape[:2]
    y0, y1, x0, x1 = h // 2 - 24, h // 2 + 24, w // 2 - 24, w // 2 + 24      # (a window is enough to tell 625 translations apart)
    best, at = -1, None
    for dy in range(-12, 13):
        for dx in range(-12, 13):
            n = int((curr[y0:y1, x0:x1] == clean_prev[y0 - dy:y1 - dy, x0 - dx:x1 - dx]).all(-1).sum())
            if n > best:
                best, at = n, (dx, dy)
    return at


@functools.lru_cache(maxsize=None)
def ingredients(size, seed):
    """Which of INGREDIENTS _mixed_pair(w, h, seed) holds, from the pixels of the pair -- not from its random draws."""
    w, h = size
    prev, curr = mixed_pair(size, seed)
    clean_prev = synth.make_prev(w, h, seed=seed)
    clean = synth.translate(clean_prev, _pan_of(clean_prev, curr), seed)
    off = np.abs(curr.astype(np.int16) - clean.astype(np.int16)).max(-1)
    found = set()
    if int(((off >= 1) & (off <= 4)).sum()) >= 200:                                     # +-1 .. +-4 levels on a band of rows
        found.add("sensor noise")
    if int((curr == synth.noise_bytes(w, h, seed + 2)).all(-1).sum()) >= 16:           # fresh noise pasted in: 4 x 4 at least
        found.add("occlusion")
    if int(((prev == 90).all(-1) & (curr == 90).all(-1)).sum()) >= 64:                 # 8 x 8 at least
        found.add("static flat area")
    if int(((prev == 50).all(-1) & (curr == 51).all(-1)).sum()) >= 400:                # 20 x 20 at least
        found.add("fade")
    return frozenset(found)


def has_fade(size, seed):
    return "fade" in ingredients(size, seed)


# ------------------------------------------------------------------ the oracle, once per session

_oracle_calls = 0


@functools.lru_cache(maxsize=None)
def oracle_vectors(size, name, semantics):
    """oracle.motion on every pixel of a pair of one of ORACLE_SIZES as int8, computed once per session and read-only."""
    global _oracle_calls
    import oracle
    assert size in ORACLE_SIZES, size
    prev, curr, _ = pairs_of(size)[name]
    _oracle_calls += 1
    mv = oracle.motion(prev, curr, semantics=oracle.INTENDED if semantics == "intended" else oracle.REFERENCE).astype(np.int8)
    return _frozen(mv)[0]


# ------------------------------------------------------------------ grids and rows

def persistent_grid_most(slots, device_cus, comm_cus):
    """lfg_motion_verdict.hpp, persistent_grid_most."""
    return slots if comm_cus <= 0 or device_cus <= comm_cus else slots // device_cus * (device_cus - comm_cus)


def shipped_grids(slots, device_cus):
    """{role: workgroups}: the persistent grids shipped configurations reach below `slots` (motion_call_policy) -- 5/8 of the
    slots with frames in flight, what a communicator's reservation leaves, and the smaller of the two."""
    grids = {"five eighths": max(1, slots * 5 // 8)}
    for c in COMM_CUS:
        grids[f"comm {c}"] = persistent_grid_most(slots, device_cus, c)
    grids["minimum"] = min(grids.values())
    return grids


SHIPPED_ROLES = tuple(shipped_grids(512, 256))


def _cross(**extra):
    return [dict(LFG_PREF_GROUPS="3", LFG_RESOLVE_GROUPS="5", LFG_DYN_PARTS_RT=str(d), **extra) for d in DYN_PARTS]


def knob_rows(slots, device_cus):
    """{name: (environment, kind)}; kind says which pairs a row runs: "all" (every size in SIZES), "lean" or "strip".  The names
    do not depend on the arguments, the shipped grids' values do."""
    rows = {}
    for role, g in shipped_grids(slots, device_cus).items():
        env = dict(LFG_PREF_GROUPS=str(g))
        if role == "minimum":                # (reached with frames in flight under a communicator: a handed-over segment in 4 parts)
            env["LFG_DYN_PARTS_RT"] = "4"
        rows[f"pref {role}"] = (env, "all")
    for g in SMALL_GRIDS:
        rows[f"pref {g}"] = (dict(LFG_PREF_GROUPS=str(g)), "all")
    for g in RESOLVE_GROUPS:
        rows[f"resolve {g}"] = (dict(LFG_RESOLVE_GROUPS=str(g)), "all")
    for d in DYN_PARTS:
        rows[f"parts {d}"] = (dict(LFG_DYN_PARTS_RT=str(d)), "all")
    for kind, flag in (("all", {}), ("all", dict(LFG_TIER_FORCE="1")), ("lean", dict(LFG_LEAN_FORCE="1")), ("strip", dict(LFG_MOTION_STRIP="1"))):
        for env in _cross(**flag):
            what = "".join(f", {k[4:].lower().replace('_', ' ')}" for k in flag)
            rows[f"cross, parts {env['LFG_DYN_PARTS_RT']}{what}"] = (env, kind)
    return rows


ROW_NAMES = tuple(knob_rows(512, 256))
