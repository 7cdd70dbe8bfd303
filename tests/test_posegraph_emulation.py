"""The pose-graph kernel's arithmetic without a GPU: tests/posegraph_emulation.cpp runs the whole optimisation
single-threaded from the functions of csrc/posegraph_device.h that the kernel calls (edge residual and system, the
controller) with the kernel's assembly and summation orders, compiled by g++ under AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program.  Every scenario class is compared with the numpy restatement:
decisions equal, numbers under the rule of tests/posegraph_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import posegraph_cases as PC
from util import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pg") / "posegraph_emulation")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "posegraph_emulation.cpp"), "-o", path])
    return path


def read_result(path, n, m):
    tok = open(path).read().split()
    head, tok = tok[:9], tok[9:]
    poses = np.array(tok[:16 * n], dtype=np.float64).reshape(n, 4, 4)
    tok = tok[16 * n:]
    conf = np.array(tok[0:2 * m:2], dtype=np.float64)
    pruned = [int(v) for v in tok[1:2 * m:2]]
    tok = tok[2 * m:]
    rows = np.array(tok[1:], dtype=np.float64).reshape(int(tok[0]), 6)
    flags, lam = [[], []], [[], []]
    for p, l, _, _, acc, fac in rows:
        flags[int(p)].append((bool(acc), bool(fac)))
        lam[int(p)].append(l)
    return dict(status=int(head[0]), iterations=[int(head[1]), int(head[2])], trials=[int(head[3]), int(head[4])],
                F0=float(head[5]), F=float(head[6]), mu=[float(head[7]), float(head[8])], poses=poses, confidence=conf,
                pruned=pruned, flags=flags, lam=lam)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_emulation_agrees_with_the_restatement(exe, tmp_path, name):
    assert PC.WIDE
    start, edges, _ = PC.build(name)
    gfile, rfile = str(tmp_path / "graph.txt"), str(tmp_path / "result.txt")
    PC.write_graph_file(gfile, name)
    out = subprocess.run([exe, gfile, rfile], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    PC.check_against_reference(name, read_result(rfile, len(start), len(edges)))
