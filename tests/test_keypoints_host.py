"""The host side of ISS keypoint detection without a GPU: csrc/icp.hip and csrc/icp_keypoints.hip compiled by g++ against
the HIP stand-in header, with the lane-independent device source (csrc/icp_iss_device.h: keys, gather, the ordered walk
over the sorted cell index, saliency, suppression, resolution; the ring kernel of csrc/kernels_outlier.hip for the
resolution's self k-NN) run one lane at a time (tests/keypoints_host_driver.cpp), under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program.  The device sort is a std::stable_sort behind one function.
Descriptors, the key layout, the packed output layout with every subset of the optional outputs, both stages and every
refusal run for real; masks, saliencies, counts and radii are compared bit for bit with the restatement's."""
import os
import subprocess

import numpy as np

import keypoints_reference as RK
import normals_reference as RN
from util import ROOT


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())


def ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def cases():
    """(points, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors).  The first is a non-empty cube (the
    driver builds its refusals on it)."""
    out = [(RN.cube(129), 0.0, 0.0, 0.975, 0.975, 5), (RN.cube(65, 5), 0.3, 0.45, 0.975, 0.975, 5),
           (RN.cube(300, 6), 0.35, 0.05, 0.975, 0.975, 5), (np.zeros((0, 3)), 0.0, 0.0, 0.975, 0.975, 5),
           (RN.cube(257, 7), 0.3, 0.0, 0.9, 0.8, 3), (RN.planar(), 0.35, 0.2, 0.975, 0.975, 5),
           (RN.collinear(), 0.0, 0.0, 0.975, 0.975, 5), (RN.collinear(), 0.6, 0.4, 0.975, 0.975, 2),
           (RN.identical(), 0.0, 0.0, 0.975, 0.975, 5), (RN.identical(), 0.1, 0.1, 0.975, 0.975, 5),
           (RN.tied_lattice(), 0.0, 0.0, 0.975, 0.975, 5), (RN.tied_lattice(), 0.55, 0.3, 2.0, 2.0, 5),
           (RN.tied_lattice(), 0.3, 0.6, 2.0, 2.0, 5),
           (RN.cube(200, 8), 0.3, 0.2, 0.0, 0.975, 5), (RN.cube(200, 8), 0.3, 0.2, 2.0, 2.0, 0),
           (RN.cube(129, 9) + np.array([1e6, -1e6, 1e6]), 0.3, 0.2, 0.975, 0.975, 5),
           (RK.dyadic_cloud(), 1.0, 0.75, 0.975, 0.975, 5)]
    out += [(RN.cube(n, 10 + n), r, r, 2.0, 2.0, 5) for n in (1, 2, 4, 5, 6) for r in (0.0, 2.0)]
    return out


def test_host_code_and_lane_independent_kernel_source_equal_the_restatement(tmp_path):
    lines = []
    cs = cases()
    keypoints = 0
    for P, rs, rn, g21, g32, mn in cs:
        ref = RK.iss_keypoints(P, rs, rn, g21, g32, mn)
        keypoints += int(ref["keep"].sum())
        lines += ["%d %s %d" % (len(P), hexes([rs, rn, g21, g32]), mn), hexes(P), ints(ref["keep"]),
                  hexes(ref["saliency"]), ints(ref["count"]), hexes(ref["radii"])]
    assert keypoints > 20
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = str(tmp_path / "keypoints_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "keypoints_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
