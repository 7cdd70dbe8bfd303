"""The host side of self k-NN and outlier removal without a GPU: csrc/icp.hip compiled by g++ against the HIP stand-in
header with CPU stand-ins for the kernel launchers (tests/outlier_host_driver.cpp), under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program.  Descriptor building, the output layout, the worklist's size,
the copy back and the argument checks run for real; the numbers are compared bit for bit with the restatement's."""
import os
import subprocess

import numpy as np

import outlier_reference as R
from util import ROOT


def hexes(a):
    return " ".join(float(x).hex() if np.isfinite(x) else ("nan" if np.isnan(x) else "inf")
                    for x in np.asarray(a, dtype=np.float64).ravel())


def ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def cases():
    rng = np.random.default_rng(41)
    g = 0.25 * np.arange(3)
    lattice = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], 1)
    dup = rng.random((90, 3))
    dup[20:50] = dup[5]
    far = rng.random((130, 3))
    far[77] = [1e6, 1e6, 1e6]
    return [(rng.random((70, 3)), 5, 2.0, 2, 0.3), (np.zeros((0, 3)), 7, 1.0, 1, 0.1), (lattice, 7, 1.0, 3, 0.25),
            (rng.random((1, 3)), 3, 1.0, 1, 0.5), (dup, 20, 2.0, 4, 0.2), (rng.random((257, 3)), 100, 1.5, 6, 0.25),
            (far, 33, 2.0, 2, 0.2), (np.tile([[1.0, 2.0, 3.0]], (40, 1)), 10, 1.0, 5, 0.1),
            (rng.random((3, 3)) * 1e-3 + 1e4, 100, 0.5, 1, 1e-3)]


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    lines = []
    cs = cases()
    for P, k, ratio, nb, radius in cs:
        idx, d2 = R.self_knn(P, k)
        s = R.statistical(P, k, ratio)
        r = R.radius(P, nb, radius)
        lines += ["%d %d %s %d %s" % (len(P), k, float(ratio).hex(), nb, float(radius).hex()), hexes(P), ints(idx),
                  hexes(d2), hexes(s["avg"]), hexes([s["mean"], s["std"], s["threshold"]]), ints(s["keep"]),
                  ints(r["count"]), ints(r["keep"])]
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = str(tmp_path / "outlier_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "outlier_host_driver.cpp"), "-o", exe])
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]


def test_ring_and_radius_kernel_source_equals_brute_force_on_the_host(tmp_path):
    """tests/outlier_kernel_emulation.cpp: the kernels' own source, one lane at a time, on the grids icp.hip builds --
    cube / shifted / tiny clouds, the tied lattice, far outliers (which must reach the worklist), planar, collinear,
    nearly collinear (extents of 1e-170 of the longest: no query may reach the worklist), identical and duplicated
    clouds, n = 1 .. 513, k = 1 .. 100, five points with colliding buckets."""
    exe = str(tmp_path / "outlier_kernel_emulation")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-x", "c++", "-I" + os.path.join(ROOT, "tests", "hip_stub"),
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "teaser-plusplus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "outlier_kernel_emulation.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "TOTAL mismatches 0" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
