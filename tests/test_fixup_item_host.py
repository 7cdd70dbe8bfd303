"""csrc/fixup_item.h compiled for the HOST (g++, no GPU): the group item of the K1 fix-up's worklist.  K1's harvest
packs an item's 16 provisional bits out of the column's transposed word (rows 32 rt + 4 h + {0..3, 8..11, 16..19,
24..27}); the fix-up reads bit q back for pair q.  Round trip for every (rt, h) over corner-case and random words, and
the row, column and flag fields are untouched by the provisional bits."""
import functools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = 400  # words: 0, all ones, the 64 single bits, then random ones


@functools.lru_cache(maxsize=None)
def output():
    out = os.path.join(tempfile.mkdtemp(prefix="fxi"), "fixup_item_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fixup_item_main.cpp"), "-o", out])
    lines = subprocess.check_output([out, str(COUNT)], text=True).splitlines()
    names = ("rt", "h", "row0", "col", "word", "row0_back", "col_back", "group", "upper15", "bits_ok", "gather_ok", "fields_ok")
    return [dict(zip(names, map(int, l.split()))) for l in lines[:-1]], list(map(int, lines[-1].split()))


def test_every_rt_h_and_word_is_covered():
    rows, _ = output()
    assert len(rows) == 4 * COUNT
    assert [(r["rt"], r["h"]) for r in rows[:4]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    words = [r["word"] for r in rows[::4]]
    assert words[0] == 0 and words[1] == 2 ** 64 - 1 and words[2:66] == [1 << b for b in range(64)]
    assert len(set(words[66:])) == COUNT - 66


def test_provisional_bits_round_trip():
    rows, offs = output()
    assert offs == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert all(r["bits_ok"] == 1 and r["gather_ok"] == 1 for r in rows)


def test_row_column_and_flag_fields_are_untouched():
    rows, _ = output()
    for r in rows:
        assert r["row0_back"] == r["row0"] and r["col_back"] == r["col"], r
        assert r["group"] == 1 and r["upper15"] == 0 and r["fields_ok"] == 1, r
