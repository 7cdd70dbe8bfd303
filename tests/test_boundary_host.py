"""The host side of boundary-point detection without a GPU: csrc/icp_boundary.hip (and the list planning of
csrc/icp_fpfh.hip it shares) compiled by g++ against the HIP stand-in header with CPU stand-ins for the launchers; the
boundary launcher calls the functions of csrc/icp_boundary_device.h -- the text the kernel compiles --
(tests/boundary_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and UndefinedBehaviorSanitizer and
run as a stand-alone program.  Validation, descriptors, pieces and passes at three values of fpfh_list_bytes, the output
layout, the optional outputs, the normals estimated inside the call (a stand-in rule the case file restates), the device
count, the copy back and every refusal run for real; the mask, the bits of max_gap and the list lengths are compared
for equality with the restatement's."""
import subprocess

import boundary_reference as R
from test_fpfh_o3d_host import stand_in_normals
from test_outlier_host import hexes, ints
from test_search_host import compile_driver


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cs = [(P, N, s, r, k, t, 0) for _, P, N, s, r, k, t in R.case_list()]
    for name in ("n65", "n257", "knn33", "n1"):  # the same clouds with normals estimated inside the call
        _, P, _, s, r, k, t = next(c for c in R.case_list() if c[0] == name)
        cs.append((P, stand_in_normals(P), s, r, k, t, 1))
    lines = []
    for P, N, s, r, k, t, est in cs:
        mask, gap, m = R.boundary_points(P, N, s, r, k, t)
        assert mask.shape == gap.shape == m.shape == (len(P),)
        lines += ["%d %d %d %s %s %d" % (len(P), s, k, float(r).hex(), float(t).hex(), est), hexes(P), hexes(N),
                  ints(mask), hexes(gap), ints(m)]
    path = tmp_path / "cases.txt"
    path.write_text("%d\n" % len(cs) + "\n".join(lines) + "\n")
    exe = compile_driver("boundary_host_driver", tmp_path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
