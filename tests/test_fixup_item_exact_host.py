"""csrc/fixup_item.h compiled for the HOST (g++, no GPU): the fix-up's write-back on the no-store route of K1.  The
fix-up packs the 16 exact bits of an item's pairs over the item's own word -- fxi::pack(row0, col, exact_bits) -- and
the replay behind a rebuild reads bit q back for pair q: packing exact bits over an item keeps row0, col and the group
flag, and fxi::bit returns the recorded bits at all 16 positions, whatever provisional bits the item carried."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 300  # no bit, every bit, the 16 single bits, their complements (at the extreme row0 / col), then random fields


@functools.lru_cache(maxsize=None)
def rows():
    out = os.path.join(tempfile.mkdtemp(prefix="fxie"), "fixup_item_exact_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fixup_item_exact_main.cpp"), "-o", out])
    names = ("row0", "col", "prov", "exact", "row0_back", "col_back", "group", "upper15", "bits_ok")
    return [dict(zip(names, map(int, l.split()))) for l in subprocess.check_output([out, str(COUNT)], text=True).splitlines()]


def test_corner_cases_and_random_fields_are_covered():
    r = rows()
    assert len(r) == COUNT
    assert [x["exact"] for x in r[:2]] == [0, 0xffff]
    assert [x["exact"] for x in r[2:18]] == [1 << q for q in range(16)]
    assert [x["exact"] for x in r[18:34]] == [0xffff ^ (1 << q) for q in range(16)]
    assert {(x["row0"], x["col"]) for x in r[:34]} == {(0, 0), (65532, 0), (0, 65535), (65532, 65535)}
    assert len({(x["row0"], x["col"], x["exact"]) for x in r[34:]}) == COUNT - 34
    assert any(x["prov"] != x["exact"] for x in r)


def test_packing_exact_bits_keeps_row_column_and_flag():
    for x in rows():
        assert x["row0_back"] == x["row0"] and x["col_back"] == x["col"], x
        assert x["group"] == 1 and x["upper15"] == 0, x


def test_bit_returns_the_recorded_bits_at_all_16_positions():
    assert all(x["bits_ok"] == 1 for x in rows())
