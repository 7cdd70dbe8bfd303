"""csrc/fixup_regions.h compiled for the HOST (g++, no GPU): K1's block decode.  For T = 1, 4, 5, 8, 9, 31, 32, 33, 157
and 1024 tiles and 1, 2, 4 column chunks per block, fxr::decode_block over blockIdx.x = 0 .. blocks - 1 (gyr and the
block count as K1's launcher computes them) produces every (row group, column group) pair of the triangular grid
exactly once and nothing else."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (1, 4, 5, 8, 9, 31, 32, 33, 157, 1024)


@functools.lru_cache(maxsize=None)
def rows():
    out = os.path.join(tempfile.mkdtemp(prefix="fxo"), "block_order_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "block_order_main.cpp"), "-o", out])
    names = ("T", "chunks", "blocks", "once", "twice", "missing", "outside")
    return [dict(zip(names, map(int, l.split()))) for l in subprocess.check_output([out] + [str(t) for t in TILES], text=True).splitlines()]


def triangle_blocks(T, chunks):
    """blocks of 4 row tiles x 8 chunks column tiles with a column tile at or right of a row tile"""
    ct = 8 * chunks
    return sum(1 for X in range((T + ct - 1) // ct) for Ig in range((T + 3) // 4) if ct * X + ct - 1 >= 4 * Ig)


def test_every_size_and_geometry_is_covered():
    assert [(r["T"], r["chunks"]) for r in rows()] == [(T, c) for T in TILES for c in (1, 2, 4)]


def test_every_block_of_the_triangular_grid_exactly_once_and_nothing_else():
    for r in rows():
        assert r["blocks"] == triangle_blocks(r["T"], r["chunks"]), r
        assert r["once"] == r["blocks"] and r["twice"] == 0 and r["missing"] == 0 and r["outside"] == 0, r
