"""The host side of RGB-D odometry without a GPU: csrc/icp_odometry.hip compiled by g++ against the HIP stand-in header
with CPU stand-ins for the launchers, which call the functions of csrc/icp_odometry_device.h -- the text the kernels
compile -- (tests/odometry_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a stand-alone program.  Validation, the records, the packing of padded rows, the
block map of all levels, the pool layout, the launch sequence, the trace and every refusal run for real; pyramids, traces,
transformations, information matrices and counts are compared for equality with the restatement's, alone and in batches."""
import subprocess

import numpy as np

import odometry_reference as R
from test_outlier_host import hexes, ints
from odometry_cxx import host_driver  # compile_driver of test_search_host, once per session


def image_numbers(a):
    return ints(a) if a.dtype.kind == "u" else hexes(a)


def row_padding(a):
    return a.strides[0] - a.shape[1] * a.itemsize * (a.shape[2] if a.ndim == 3 else 1)


def case_lines(cs):
    p, o, r = cs.pair, cs.opt, R.result(cs.name)
    h, w = p.source_depth.shape
    lines = ["%d %d %d %d %d %d %d %d %s" % (w, h, 0 if p.source_depth.dtype == np.uint16 else 1,
                                             1 if p.source_color.dtype == np.uint8 else 2, p.jacobian, row_padding(p.source_depth),
                                             row_padding(p.source_color), len(o.iterations), ints(o.iterations)),
             hexes(p.K) + " " + hexes(p.odo_init) + " " + hexes([p.depth_scale, p.depth_trunc, o.depth_diff_max, o.depth_min, o.depth_max])]
    lines += [image_numbers(a) for a in (p.source_depth, p.source_color, p.target_depth, p.target_color)]
    lines += [hexes(R.pyramid(cs.name)), "%d %d %d" % (r.success, r.count, r.iterations), hexes(r.transformation), hexes(r.information)]
    for t in r.trace:
        lines.append("%d %d %d %d %s %s %s %s" % (t["level"], t["executed"], t["count"], t["failed"], hexes([t["e"]]), hexes(t["A"]),
                                                  hexes(t["g"]), hexes(t["pose"])))
    return lines


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cs = [c for c in R.cases().values() if c.host]
    assert any(row_padding(c.pair.source_depth) for c in cs) and {c.pair.jacobian for c in cs} == {0, 1}
    assert {c.pair.source_depth.dtype for c in cs} == {np.dtype(np.uint16), np.dtype(np.float32)}
    assert any(not R.result(c.name).success for c in cs) and any(R.result(c.name).count == 0 for c in cs)
    lines = [str(len(cs))]
    for c in cs:
        lines += case_lines(c)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = host_driver()
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
