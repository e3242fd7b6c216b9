"""The geometry of tests/big_views.py without a GPU: every view that tests/test_gpu_big_views.py makes fits the arena, and every
offset that a 32-bit miscalculation of one of its byte offsets can give still lies inside the arena -- a wrong byte, never a fault
-- and is another number than the true offset wherever the miscalculation overflows, so that it is a wrong byte.  CPU only."""
import pytest

from tests import big_views as bv

LOWEST, HIGHEST = -bv.BASE, bv.ARENA - bv.BASE - 16       # offsets from a view's start that a 16-byte access may take


def views():
    """(rows, row bytes, plane kind, geometry) of every big view of the GPU tests."""
    out = set()
    for name, op, geometry in bv.tall_cases():
        o = bv.operands_of(name, *bv.IMAGE)[op]
        out.add((o.rows, o.row_bytes, bv.PLANE[o.kind], geometry))
    for name, op, w, h in bv.plane_cases():
        o = bv.operands_of(name, w, h)[op]
        out.add((o.rows, o.row_bytes, bv.PLANE[o.kind], "pitch31"))
    return sorted(out)


def test_the_geometries_are_the_stated_ones():
    assert bv.ARENA == 6_710_886_400
    assert bv.pitch_of("tall4", 40) == 110_154_256 and bv.pitch_of("tall2", 40) == 55_090_576
    for g, kind, bump in (("tall2_4", "frame", 4), ("tall4_4", "byte", 1), ("tall2_4", "uv", 2)):
        assert bv.pitch_of(g, 40, kind) == bv.pitch_of(g[:-2], 40, kind) + bump
    for rows in (2, 13, 20, 40, 60, 80):
        for g, span in (("tall2", 2 ** 31), ("tall4", 2 ** 32)):
            p = bv.pitch_of(g, rows)
            assert p % 16 == 0 and (rows - 1) * p >= span + 2 ** 20 > (rows - 1) * (p - 16)
    assert bv.pitch_of("pitch31", 2) == 2 ** 31 + 64
    assert {v[3] for v in views()} == set(bv.GEOMETRIES)


def test_the_pitch31_planes_have_two_rows():
    for name, op, w, h in bv.plane_cases():
        assert bv.operands_of(name, w, h)[op].rows == 2, (name, op)
    assert "frame_ssim" not in {c[0] for c in bv.plane_cases()}     # the call that needs more rows than two has no plane


@pytest.mark.parametrize("rows,row_bytes,kind,geometry", views())
def test_every_alias_lies_inside_the_arena_and_is_a_wrong_byte(rows, row_bytes, kind, geometry):
    assert bv.fits(geometry, rows, row_bytes, kind)
    assert bv.BASE + (rows - 1) * bv.pitch_of(geometry, rows, kind) + row_bytes + bv.GUARD <= bv.ARENA
    crossed = set()
    for name, true, alias, same in bv.aliases(geometry, rows, row_bytes, kind):
        assert LOWEST <= alias <= HIGHEST, (name, true, alias)
        assert (alias == true) == same, (name, true, alias)
        if not same:
            crossed.add(name)
    # what each geometry is there to cross
    want = {"tall2": {"i32(y * P + x)", "i32(y * P) + x"}, "tall4": set(bv.ALIASES) - {"y * i32(P) + x"}, "pitch31": set(bv.ALIASES) - {"u32(y * P + x)", "u32(y * P) + x"}}
    assert crossed >= want[geometry.split("_")[0]], (geometry, crossed)


def test_the_figures_of_the_40_row_kib_view():
    """64 x 40 RGBA8 rows are 256 bytes; with 1 KiB rows over all geometries the lowest alias is -2,147,483,584 (row 1 of pitch31 with the
    pitch taken as an int) and the highest 4,296,017,163 (the last byte of tall4_4's last row, which does not wrap)."""
    found = [a for g in bv.GEOMETRIES for _, _, a, _ in bv.aliases(g, 2 if g == "pitch31" else 40, 1024)]
    assert (min(found), max(found)) == (-2_147_483_584, 4_296_017_163)
    assert LOWEST <= min(found) and max(found) <= HIGHEST
