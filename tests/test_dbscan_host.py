"""The host side of DBSCAN clustering without a GPU: csrc/icp.hip and csrc/icp_cluster.hip compiled by g++ against the
HIP stand-in header, with the lane-independent device source (csrc/icp_iss_device.h: keys, gather, the ordered walk over
the sorted cell index; csrc/icp_dbscan_device.h: count, union, flatten, label and the union-find) run one lane at a time
(tests/dbscan_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program.  The
device sort is a std::stable_sort and the device scan a loop, each behind one function; the compare-and-swap is a plain
one.  Descriptors, the key layout, the packed output layout with every subset of the optional outputs, the batch in both
orders and every refusal run for real; labels, counts, roots and cluster counts are compared with the restatement's."""
import os
import subprocess

import numpy as np

import dbscan_reference as RD
from util import ROOT


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())


def ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel()) or ""


def cases():
    """(points, eps, min_points, expected).  The first is a non-empty slab (the driver builds its refusals on it)."""
    out = [(P, eps, mp, RD.expected(name)) for name, (P, eps, mp) in RD.builders().items()]
    rng = np.random.default_rng(26)
    extra = [(np.zeros((0, 3)), 0.5, 3), (RD.random_lattice(rng, 1), 0.5, 1), (RD.random_lattice(rng, 1), 0.5, 2),
             (RD.random_lattice(rng, 2, side=2), 0.6, 1), (RD.random_lattice(rng, 2, side=2), 0.6, 2),
             (RD.lattice_slab(), 0.0, 1), (RD.lattice_slab(), 1e-200, 1),  # inactive: eps * eps is not > 0
             (RD.lattice_slab(), 0.3, 1), (RD.lattice_slab(), 0.3, 190),   # every point core; all noise (n + 1)
             (RD.random_lattice(rng, 255), 0.6, 4), (RD.random_lattice(rng, 256), 0.6, 4),
             (RD.random_lattice(rng, 257), 0.6, 4)]
    out += [(P, eps, mp, RD.dbscan(P, eps, mp)) for P, eps, mp in extra]
    return out


def test_host_code_and_lane_independent_kernel_source_equal_the_restatement(tmp_path):
    lines = []
    cs = cases()
    clusters = noise = 0
    for P, eps, mp, (labels, counts, roots, c) in cs:
        clusters += c
        noise += int((labels < 0).sum())
        lines += ["%d %s %d %d" % (len(P), hexes([eps]), mp, c), hexes(P), ints(labels), ints(counts), ints(roots)]
    assert clusters > 20 and noise > 100
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = str(tmp_path / "dbscan_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dbscan_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
