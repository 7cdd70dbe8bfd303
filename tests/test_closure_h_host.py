"""csrc/closure_h.h compiled for the HOST (g++, no GPU): the H rule the closure's verdict launch applies to its full rows,
on the cases of the numpy model (tests/closure_full_rows_model.py), plain and under -fsanitize=address,undefined -- a
stand-alone program, nothing loaded into python."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import closure_full_rows_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(m, kind) for m in M.SIZES for kind in M.KINDS]


@functools.lru_cache(maxsize=None)
def case_file():
    path = os.path.join(tempfile.mkdtemp(prefix="clh"), "cases.bin")
    with open(path, "wb") as f:
        for m, kind in CASES:
            adj, deg = M.case(m, kind)
            pool, _ = M.pairs_launch(adj, 16)
            f.write(np.int32(m).tobytes())
            f.write(deg.astype(np.uint16).tobytes())
            f.write(np.ascontiguousarray(pool[:m, :(m + 63) // 64]).tobytes())
        f.write(np.int32(0).tobytes())
    return path


@functools.lru_cache(maxsize=None)
def run(sanitize):
    out = os.path.join(tempfile.mkdtemp(prefix="clh"), "closure_h_main")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags,
                           "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "closure_h_main.cpp"), "-o", out])
    lines = subprocess.check_output([out, case_file()], text=True).splitlines()
    return [np.array(l.split(), np.int64) for l in lines]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_header_rule_equals_the_definition_on_every_case(sanitize):
    got = run(sanitize)
    assert len(got) == len(CASES)
    for (m, kind), h in zip(CASES, got):
        adj, deg = M.case(m, kind)
        assert np.array_equal(h, M.h_definition(adj, deg)), (m, kind)
