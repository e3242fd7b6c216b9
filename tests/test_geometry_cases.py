"""tests/geometry_cases.py held to what it claims, without a GPU: the rows parse, the grids are derived and stay within the
slots, the pairs hold what the GPU tests rely on, the oracle is asked once per pair."""
import numpy as np
import pytest

from linux_fg_amd import synth
from tests import geometry_cases as gc

KNOWN_KNOBS = {"LFG_PREF_GROUPS", "LFG_RESOLVE_GROUPS", "LFG_DYN_PARTS_RT", "LFG_TIER_FORCE", "LFG_LEAN_FORCE", "LFG_MOTION_STRIP"}


@pytest.mark.parametrize("slots,cus", [(512, 256), (608, 304)])
def test_knob_rows_parse_and_grids_stay_within_the_slots(slots, cus):
    rows = gc.knob_rows(slots, cus)
    assert tuple(rows) == gc.ROW_NAMES and len(set(gc.ROW_NAMES)) == len(gc.ROW_NAMES)
    for name, (env, kind) in rows.items():
        assert kind in ("all", "lean", "strip") and set(env) <= KNOWN_KNOBS, name
        values = {k: int(v) for k, v in env.items()}                       # atoi in lfg_context_create: decimal integers
        assert all(str(v) == env[k] and v > 0 for k, v in values.items()), (name, env)
        assert 1 <= values.get("LFG_PREF_GROUPS", 1) <= slots, (name, env)
        assert values.get("LFG_DYN_PARTS_RT", 4) in (4, 8), (name, env)
        assert (kind == "lean") == ("LFG_LEAN_FORCE" in env) and (kind == "strip") == ("LFG_MOTION_STRIP" in env), name
    pref = {int(env["LFG_PREF_GROUPS"]) for env, _ in rows.values() if "LFG_PREF_GROUPS" in env}
    assert set(gc.SMALL_GRIDS) <= pref
    assert {int(env["LFG_RESOLVE_GROUPS"]) for env, _ in rows.values() if "LFG_RESOLVE_GROUPS" in env} == set(gc.RESOLVE_GROUPS)
    for kind in ("all", "lean", "strip"):                                   # the cross, both parts, for each kind
        crossed = [env for env, k in rows.values() if k == kind and env.get("LFG_PREF_GROUPS") == "3" and env.get("LFG_RESOLVE_GROUPS") == "5"]
        assert {env["LFG_DYN_PARTS_RT"] for env in crossed} == {"4", "8"}, kind
    assert sum("LFG_TIER_FORCE" in env for env, _ in rows.values()) == 2


def test_shipped_grids_are_derived_from_the_slots():
    g = gc.shipped_grids(512, 256)
    assert tuple(g) == gc.SHIPPED_ROLES
    assert g == {"five eighths": 320, "comm 8": 496, "comm 16": 480, "comm 24": 464, "comm 32": 448, "minimum": 320}
    other = gc.shipped_grids(608, 304)                                       # two workgroups on each of 304 CUs
    assert other == {"five eighths": 380, "comm 8": 592, "comm 16": 576, "comm 24": 560, "comm 32": 544, "minimum": 380}
    for slots, cus in ((512, 256), (608, 304), (256, 256), (8, 8)):
        for role, v in gc.shipped_grids(slots, cus).items():
            assert 0 < v <= slots, (slots, cus, role, v)
    assert gc.persistent_grid_most(512, 256, 0) == 512 and gc.persistent_grid_most(8, 8, 8) == 8


@pytest.mark.parametrize("size", gc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mixed_pairs_hold_every_ingredient_between_them(size):
    found = {seed: gc.ingredients(size, seed) for seed in gc.MIXED_SEEDS}
    assert set().union(*found.values()) == set(gc.INGREDIENTS), found
    assert any(gc.has_fade(size, seed) for seed in gc.MIXED_SEEDS)
    for seed in gc.MIXED_SEEDS:
        prev, curr = gc.mixed_pair(size, seed)
        assert prev.shape == curr.shape == (size[1], size[0], 4) and not prev.flags.writeable and not curr.flags.writeable
    assert gc.ingredients(size, 9129) == set()                              # (a seed that draws none of them: the reading is not vacuous)


def test_noise_pair_is_uncorrelated():
    for size in gc.SIZES:
        a, b = gc.noise_pair(size)
        assert a.shape == (size[1], size[0], 4)
        assert (a == b).mean() < 0.01 and len(np.unique(a)) == 256
        for dx, dy in ((0, 0), (3, -2), (-16, 16)):                         # ... under translations too: no candidate matches
            assert (a[20:60, 20:60] == b[20 + dy:60 + dy, 20 + dx:60 + dx]).all(-1).sum() == 0


def test_hand_over_pair_shows_the_hints_a_pan_and_the_segments_noise():
    w, h = gc.HAND_OVER_SIZE
    assert (w % gc.TILE_W, h % gc.TILE_H) == (0, 0) and (w // gc.TILE_W) * (h // gc.TILE_H) * (gc.TILE_H // gc.SEGMENT_ROWS) == 308
    prev, curr = gc.hand_over_pair()
    dx, dy = gc.HAND_OVER_SHIFT
    origins = gc.hint_sample_origins(w, h)
    assert len(origins) == 256 and origins[0] == (w // 32 - 4, h // 32 - 4) and origins[-1] == (31 * w // 32 - 4, 31 * h // 32 - 4)
    for bx, by in origins:                                                  # every sample block: curr(q) = prev(q - shift), exactly
        assert 0 <= bx - dx and bx + 8 <= w and 0 <= by - dy and by + 8 <= h      # (the block's source lies inside prev)
        assert (curr[by:by + 8, bx:bx + 8] == prev[by - dy:by - dy + 8, bx - dx:bx - dx + 8]).all()
    # ... while every segment (16 rows of a 56-column tile) holds fresh noise: positions whose block matches nothing in prev
    fresh = (curr == synth.noise_bytes(w, h, 777)).all(-1)
    for ty in range(0, h, gc.SEGMENT_ROWS):
        for tx in range(0, w, gc.TILE_W):
            assert fresh[ty:ty + gc.SEGMENT_ROWS, tx:tx + gc.TILE_W].mean() > 0.4, (tx, ty)
    assert 0.6 < fresh.mean() < 0.85                                        # islands: a quarter of the frame


def test_the_queue_size_has_whole_tiles_where_the_other_sizes_share_theirs():
    """prefilter_plan: a frame with fewer tiles than half the slots has every tile shared between units, and only a unit that holds
    a whole tile hands a segment over."""
    slots = 512
    assert all(2 * gc.tiles_of(size) <= slots for size in gc.SIZES), [gc.tiles_of(s) for s in gc.SIZES]
    assert 2 * gc.tiles_of(gc.QUEUE_SIZE) > slots and gc.tiles_of(gc.QUEUE_SIZE) == 17 * 16
    w, h = gc.QUEUE_SIZE
    assert w % gc.TILE_W and h % gc.TILE_H and h % gc.SEGMENT_ROWS
    assert set(gc.pairs_of(gc.QUEUE_SIZE)) == {f"mixed {gc.QUEUE_MIXED_SEED}", "hand-over", "scattered"}
    assert "occlusion" in gc.ingredients(gc.QUEUE_SIZE, gc.QUEUE_MIXED_SEED)      # segments without a match inside the frame
    prev, curr = gc.hand_over_pair(gc.QUEUE_SIZE)
    dx, dy = gc.HAND_OVER_SHIFT
    for bx, by in gc.hint_sample_origins(w, h):
        assert (curr[by:by + 8, bx:bx + 8] == prev[by - dy:by - dy + 8, bx - dx:bx - dx + 8]).all()
    assert (curr == synth.noise_bytes(w, h, 777)).all(-1).mean() > 0.9


def test_scattered_pair_has_one_unmatched_segment_in_each_of_54_whole_tiles():
    w, h = gc.QUEUE_SIZE
    prev, curr = gc.scattered_pair()
    dx, dy = gc.SCATTERED_SHIFT
    patches = gc.scattered_patches()
    clean = np.ones((h, w), bool)
    segments = set()
    for x0, y0, pw, ph in patches:
        clean[y0:y0 + ph, x0:x0 + pw] = False
        # pixels whose 8 x 8 block (origin: the pixel - 4) touches the patch: all in one segment of one tile, away from the rim
        px0, px1, py0, py1 = x0 - 3, x0 + pw + 3, y0 - 3, y0 + ph + 3
        assert px0 // gc.TILE_W == px1 // gc.TILE_W and py0 // gc.SEGMENT_ROWS == py1 // gc.SEGMENT_ROWS, (x0, y0)
        tx, ty = px0 // gc.TILE_W, py0 // gc.TILE_H
        assert 1 <= tx < w // gc.TILE_W - 1 and 1 <= ty < h // gc.TILE_H - 1                   # a whole interior tile
        segments.add((tx, ty, py0 // gc.SEGMENT_ROWS))
        assert (curr[y0:y0 + ph, x0:x0 + pw] == synth.noise_bytes(w, h, 5454)[y0:y0 + ph, x0:x0 + pw]).all()
    assert len(segments) == len(patches) == 54 and len({(tx, ty) for tx, ty, _ in segments}) == 54
    assert 54 * 2 <= (gc.tiles_of(gc.QUEUE_SIZE) * 4 // 4) // 2                               # fewer than the queue holds, in 8 parts (two entries) each
    inner = np.s_[16:h - 16, 16:w - 16]
    moved = np.zeros_like(curr)
    moved[16:h - 16, 16:w - 16] = prev[16 - dy:h - 16 - dy, 16 - dx:w - 16 - dx]
    assert (curr[inner] == moved[inner]).all(-1)[clean[inner]].all()                          # everything else is the pan


def test_lean_and_strip_pairs_are_the_existing_cases():
    pairs = gc.lean_pairs()
    assert set(pairs) == {"pan", "everything the prefilter treats differently"}
    w, h = gc.LEAN_SIZE
    for prev, curr in pairs.values():
        assert prev.shape == curr.shape == (h, w, 4) and prev.flags.c_contiguous and curr.flags.c_contiguous
    assert w % gc.TILE_W and h % gc.TILE_H and h % gc.SEGMENT_ROWS
    prev, curr = pairs["pan"]
    assert (curr[100:200, 100:200] == prev[103:203, 95:195]).all()          # _lean_cases' pan by (5, -3)
    name, prev, curr, shift = gc.strip_pair()
    assert shift[0] != 0 and shift[1] != 0 and prev.shape == (420, 700, 4)


def test_the_oracle_is_asked_once_per_pair():
    size = gc.ORACLE_SIZES[0]
    before = gc._oracle_calls
    a = gc.oracle_vectors(size, "noise", "reference")
    first = gc._oracle_calls
    b = gc.oracle_vectors(size, "noise", "reference")
    assert a is b and gc._oracle_calls == first and first - before <= 1
    assert a.dtype == np.int8 and a.shape == (size[1], size[0], 2) and not a.flags.writeable
    with pytest.raises(ValueError):
        a[0, 0, 0] = 1
    with pytest.raises(AssertionError):
        gc.oracle_vectors(gc.SIZES[2], "noise", "reference")                # (616 x 448 goes against the literal kernel)
    assert set(gc.ORACLE_SIZES) == set(sorted(gc.SIZES, key=lambda s: s[0] * s[1])[:2])
