"""The host side of normal estimation without a GPU: csrc/icp.hip and csrc/icp_normals.hip compiled by g++ against the
HIP stand-in header, with the lane-independent device source (csrc/icp_cov_device.h, the ring kernel's covariance
consumer) run one lane at a time (tests/normals_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer,
as a stand-alone program.  Descriptors, the packed output layout with every subset of the optional outputs, the routing
of the self-estimating point-to-plane entry and every refusal run for real; normals, covariances and eigenvalues are
compared bit for bit with the restatement's.  The scan kernel's wave merge cannot be emulated one lane at a time and
does not run here (no query of these inputs reaches the worklist; the driver asserts it).  The driver also counts the
worklist entries of the ring search on outlier_reference.planted_cloud() at ring cap 4: some at k = 10, none at
k = 30, which is what tests/test_gpu_normals.py relies on."""
import os
import subprocess

import numpy as np

import normals_reference as RN
import outlier_reference as RO
from util import ROOT


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())


def cases():
    """(points, search, radius, max_nn, orient, ref): cube, planar, collinear, identical and tied-lattice clouds,
    n = 1, 2, 3, 63, 64, 65, 129, max_nn = 3, 32, 33, 100; an empty cloud in the middle."""
    ref = (0.4, 0.6, 5.0)
    out = [(RN.cube(129), 0, 0.3, 32, 1, ref), (RN.cube(65, 5), 1, 0.0, 33, 2, ref), (RN.cube(64, 6), 0, 0.25, 3, 0, ref),
           (np.zeros((0, 3)), 0, 0.3, 30, 0, ref), (RN.planar(), 0, 0.35, 100, 2, ref), (RN.planar(63), 1, 0.0, 12, 1, ref),
           (RN.collinear(), 1, 0.0, 32, 0, ref), (RN.collinear(), 0, 0.4, 33, 1, ref), (RN.identical(), 0, 0.1, 100, 2, ref),
           (RN.identical(), 1, 0.0, 3, 1, (0.3, -1.25, 7.0)), (RN.tied_lattice(), 0, 0.25 * np.sqrt(2.5), 100, 0, ref),
           (RN.tied_lattice(), 1, 0.0, 100, 1, ref), (RN.tied_lattice(), 0, 0.3, 8, 2, ref)]
    out += [(RN.cube(n, 10 + n), s, 0.6, 3 + n, 1, ref) for n in (1, 2, 3) for s in (0, 1)]
    return out


def test_host_code_and_lane_independent_kernel_source_equal_the_restatement(tmp_path):
    lines = []
    cs = cases()
    for P, search, radius, max_nn, orient, ref in cs:
        N, Cv, E, _ = RN.estimate_normals(P, search, radius, max_nn, orient, ref)
        lines += ["%d %d %d %d %s %s" % (len(P), search, max_nn, orient, float(radius).hex(), hexes(ref)), hexes(P),
                  hexes(N), hexes(Cv), hexes(E)]
    path = tmp_path / "cases.txt"
    planted, _ = RO.planted_cloud()  # the driver counts the ring search's worklist entries on it (k = 10 and 30)
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n%d\n%s\n" % (len(planted), hexes(planted)))
    exe = str(tmp_path / "normals_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "normals_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
