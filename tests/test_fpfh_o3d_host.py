"""The host side of the Open3D-form FPFH without a GPU: csrc/icp_fpfh.hip compiled by g++ against the HIP stand-in header
with CPU stand-ins for the launchers that call the functions of csrc/icp_fpfh_device.h -- the text the kernels compile
-- (tests/fpfh_o3d_host_driver.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program with
-ffp-contract=off.  Descriptors, pieces and passes at four values of fpfh_list_bytes, the layouts, the optional outputs,
the normals estimated inside the call (a stand-in rule the case file restates), the copy back and the argument refusals
run for real; SPFH and FPFH rows are compared for equality on hexadecimal floats with the restatement's."""
import subprocess

import numpy as np

import fpfh_o3d_reference as R
from test_outlier_host import hexes
from test_search_host import compile_driver


def stand_in_normals(P):
    """What the driver's normals launchers write: (x + 1, y - 2, z + 0.5) over its length."""
    v = P + np.array([1.0, -2.0, 0.5])
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v / ln[:, None]


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cs = [(P, N, s, r, k, 0) for _, P, N, s, r, k in R.case_list()]
    for name in ("n65", "n257", "lattice_knn", "n1"):  # the same clouds with normals estimated inside the call
        _, P, _, s, r, k = next(c for c in R.case_list() if c[0] == name)
        cs.append((P, stand_in_normals(P), s, r, k, 1))
    lines = []
    for P, N, s, r, k, est in cs:
        F, H = R.compute_fpfh_feature(P, N, s, r, k)
        assert F.shape == H.shape == (len(P), 33)
        lines += ["%d %d %d %s %d" % (len(P), s, k, float(r).hex(), est), hexes(P), hexes(N), hexes(F), hexes(H)]
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = compile_driver("fpfh_o3d_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
