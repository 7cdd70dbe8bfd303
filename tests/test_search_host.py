"""The host side of the neighbour search between two clouds without a GPU: csrc/icp_search.hip compiled by g++ against
the HIP stand-in header with CPU stand-ins for the kernel launchers (tests/search_host_driver.cpp), and the source of its
kernels run one thread at a time (tests/search_kernel_emulation.cpp), both under AddressSanitizer and
UndefinedBehaviorSanitizer as stand-alone programs.  Descriptor building, the output layouts, the worklist's size, the
count-then-fill halves of the radius search, the copy back and the argument checks run for real; the numbers are compared
for equality with the restatement's."""
import os
import subprocess

import numpy as np

import search_reference as S
from test_outlier_host import hexes, ints
from util import ROOT


def compile_driver(name, tmp_path):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe])
    return exe


def cases():
    """(data, query, k, radius, max_nn): the first one serves the refusals (both sides non-empty)."""
    rng = np.random.default_rng(43)
    P = rng.random((70, 3))
    dup = rng.random((90, 3))
    dup[20:50] = dup[5]
    far = rng.random((130, 3)) * 1.2 - 0.1
    far[77] = [1e6, 1e6, 1e6]
    none = np.zeros((0, 3))
    return [(P, rng.random((37, 3)), 5, 0.3, 4), (none, rng.random((9, 3)), 7, 0.1, 3), (P, none, 3, 0.2, 2),
            (S.lattice(3), S.lattice_centres(3), 8, 0.25, 8), (S.lattice(3), S.lattice(3), 7, 0.25, 33),
            (rng.random((1, 3)), rng.random((65, 3)), 3, 0.6, 1), (dup, dup[::2] + 0.0, 20, 0.2, 40),
            (rng.random((257, 3)), far, 100, 0.25, 100), (np.tile([[1.0, 2.0, 3.0]], (40, 1)), P[:3] + [1.0, 2.0, 2.5], 10, 0.9, 5),
            (rng.random((3, 3)) * 1e-3 + 1e4, rng.random((4, 3)) * 1e-3 + 1e4, 100, 1e-3, 100), (none, none, 1, 1.0, 1)]


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    lines = []
    cs = cases()
    for P, Q, k, radius, max_nn in cs:
        kidx, kd2 = S.knn_search(P, Q, k)
        hidx, hd2, hcnt = S.hybrid_search(P, Q, radius, max_nn)
        ridx, rd2, splits = S.radius_search(P, Q, radius)
        lines += ["%d %d %d %s %d %d" % (len(P), len(Q), k, float(radius).hex(), max_nn, len(ridx)), hexes(P), hexes(Q),
                  ints(kidx), hexes(kd2), ints(hidx), hexes(hd2), ints(hcnt), ints(np.diff(splits)), ints(ridx),
                  hexes(rd2)]
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = compile_driver("search_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]


def test_search_kernel_source_equals_brute_force_on_the_host(tmp_path):
    """tests/search_kernel_emulation.cpp: the ring, hybrid, count, fill and rank kernels' own source, one thread at a
    time, on the grids icp_host.h builds over the data: queries inside the box, on its faces, one, three and five cells
    outside each side (r0 = 1, 3, 5 with 4 rings), a corner, 1e6 extents away (which must reach the worklist), at a
    lattice's points and cell centres (which must not); planar, collinear, identical and tiny shifted data, n_data =
    1 .. 513, k = 1 .. 100, both list capacities, ring caps 4, 1 and 0, five points with colliding buckets.  The scan
    kernel's shuffle merge and the prefix kernel are not emulated.  With the data cloud as the query set (a cube, the
    7^3 lattice, a cloud with two far outliers, n = 1 .. 257, k = 1, 32, 33, 100, ring caps 4 and 1) the self ring
    kernel and the two-cloud ring kernel give identical rows and worklists."""
    exe = compile_driver("search_kernel_emulation", tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "TOTAL mismatches 0" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
