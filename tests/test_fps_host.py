"""The host side of farthest-point down-sampling without a GPU: csrc/icp.hip, csrc/icp_outlier.hip (the options) and
csrc/icp_fps.hip compiled by g++ against the HIP stand-in header, with the two launchers replaced by serial loops over
the source of csrc/icp_fps_device.h (tests/fps_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer,
as a stand-alone program.  The descriptors, the route split at fps_resident_max (its default, 0 and 64), the packed
output layout with every subset of the optional outputs, the batch in both orders and every refusal run for real;
indices, sel_dist and final_dist are compared bit for bit with the restatement's."""
import os
import subprocess

import numpy as np

import fps_reference as RF
from util import ROOT


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())


def ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel()) or ""


def cases():
    """(points, K, start).  The first is a non-empty cloud with K >= 1 (the driver builds its refusals on it)."""
    rng = np.random.default_rng(27)
    return [(RF.lattice(rng, 65), 9, 3), (np.zeros((0, 3)), 0, 0), (RF.lattice(rng, 5), 0, 0), (RF.lattice(rng, 1), 1, 0),
            (RF.lattice(rng, 2), 2, 1), (RF.lattice(rng, 64), 64, 63), (RF.gaussian(rng, 257), 40, 0),
            (RF.planted(1025, 1024), 7, 0), (RF.planted(2049, 1023), 12, 2048), (RF.lattice(rng, 3000), 33, 1500),
            (RF.identical(), 5, 7), (RF.three_positions(), 6, 4), (RF.planted(10241, 10240), 3, 5)]


def test_host_code_and_lane_independent_device_source_equal_the_restatement(tmp_path):
    lines = []
    cs = cases()
    repeats = 0
    for P, K, s in cs:
        index, sel, fin = RF.fps(P, K, s)
        repeats += K - len(set(index.tolist()))
        lines += ["%d %d %d" % (len(P), K, s), hexes(P), ints(index), hexes(sel), hexes(fin)]
    assert repeats >= 4 + 3  # the identical cloud, the three positions (and a lattice with K = n) repeat their last sample
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = str(tmp_path / "fps_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fps_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
