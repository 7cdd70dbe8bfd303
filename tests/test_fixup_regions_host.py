"""csrc/fixup_regions.h compiled for the HOST (g++, no GPU): the region arena of the K1 fix-up.  K1 writes one region
per cell (row tile, column chunk) of the upper triangle, wherever its launch geometry put the wave that owns the cell;
the fix-up's wave of a row tile reads that tile's cells as one run.  For T = 1 .. 45 tiles and 1, 2, 4 column chunks
per block: every upper-triangle cell is owned by exactly one (block, wave, chunk) of K1's launch grid -- through K1's
own block decode, XCD remap included --, the fix-up's enumeration of a tile visits exactly the tile's cells, and the
arena covers the largest index."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def rows():
    out = os.path.join(tempfile.mkdtemp(prefix="fxr"), "fixup_regions_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fixup_regions_main.cpp"), "-o", out])
    names = ("T", "chunks", "cells", "once", "twice", "unowned", "outside", "max_index", "arena_regions", "fixup_ok")
    return [dict(zip(names, map(int, l.split()))) for l in subprocess.check_output([out, "1", "45"], text=True).splitlines()]


def triangle_cells(T):
    """cells (I, Xc): chunk Xc = column tiles 8 Xc .. 8 Xc + 7, in the upper triangle where one of them is >= I"""
    nch = (T + 7) // 8
    return sum(1 for I in range(T) for Xc in range(nch) if 8 * Xc + 7 >= I)


def test_every_geometry_is_covered():
    got = rows()
    assert [(r["T"], r["chunks"]) for r in got] == [(T, c) for T in range(1, 46) for c in (1, 2, 4)]


def test_every_upper_triangle_cell_has_exactly_one_owner():
    for r in rows():
        assert r["cells"] == triangle_cells(r["T"]), r
        assert r["once"] == r["cells"] and r["twice"] == 0 and r["unowned"] == 0 and r["outside"] == 0, r


def test_fixup_enumeration_visits_exactly_the_tiles_cells():
    assert all(r["fixup_ok"] == 1 for r in rows())


def test_arena_covers_the_largest_index_and_does_not_depend_on_the_geometry():
    for r in rows():
        assert r["max_index"] == r["cells"] - 1 and r["arena_regions"] == r["cells"], r
    by_T = {}
    for r in rows():
        by_T.setdefault(r["T"], set()).add(r["arena_regions"])
    assert all(len(v) == 1 for v in by_T.values())
    # the triangular prefix is about half the T x n_chunks rectangle at the bench size (T = 157 has 1677 cells)
    assert triangle_cells(157) == 1677 and 157 * 20 == 3140
