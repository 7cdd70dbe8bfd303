"""The host side of depth odometry without a GPU: csrc/icp_depth_odometry.hip compiled by g++ against the HIP stand-in
header with CPU stand-ins for the launchers, which call the functions of csrc/icp_depth_odometry_device.h -- the text the
kernels compile -- (tests/depth_odometry_host_driver.cpp).  Built with -ffp-contract=off under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a stand-alone program.  Validation, the records, the packing of padded rows, the
block map of all levels, the pool layout, the launch sequence, the trace and every refusal with its text run for real;
pyramids, traces, transformations, information matrices, measures and counts are compared for equality with the
restatement's, alone and in batches."""
import pathlib
import subprocess
import tempfile

import numpy as np

import depth_odometry_reference as R
from test_outlier_host import hexes, ints
from test_search_host import compile_driver


def image_numbers(a):
    return ints(a) if a.dtype.kind == "u" else hexes(a)


def row_padding(a):
    return a.strides[0] - a.shape[1] * a.itemsize


def case_lines(cs):
    p, o, r = cs.pair, cs.opt, R.result(cs.name)
    h, w = p.source_depth.shape
    assert row_padding(p.source_depth) == row_padding(p.target_depth)
    lines = ["%d %d %d %d %d %s" % (w, h, 0 if p.source_depth.dtype == np.uint16 else 1, row_padding(p.source_depth),
                                    len(o.iterations), ints(o.iterations)),
             hexes(p.K) + " " + hexes(p.init) + " " + hexes([p.depth_scale, o.trunc, o.delta, o.depth_min, o.depth_max,
                                                             o.relative_rmse, o.relative_fitness])]
    lines += [image_numbers(a) for a in (p.source_depth, p.target_depth)]
    lines += [hexes(R.pyramid(cs.name)), "%d %d %d %d %s" % (r.success, r.count, r.iterations, r.converged_levels,
                                                              hexes([r.fitness, r.inlier_rmse])),
              hexes(r.transformation), hexes(r.information)]
    for t in r.trace:
        lines.append("%d %d %d %d %d %s %s %s %s" % (t["level"], t["executed"], t["count"], t["failed"], t["converged"],
                                                     hexes([t["e"]]), hexes(t["A"]), hexes(t["g"]), hexes(t["pose"])))
    return lines


def test_host_code_is_clean_and_equal_to_the_restatement(tmp_path):
    cs = [c for c in R.cases().values() if c.host]
    res = {c.name: R.result(c.name) for c in cs}
    assert any(row_padding(c.pair.source_depth) for c in cs)                                     # padded rows
    assert {c.pair.source_depth.dtype for c in cs} == {np.dtype(np.uint16), np.dtype(np.float32)}  # both formats
    assert any(not r.success and r.count == 0 for r in res.values())                             # a failed pair
    assert any(r.converged_levels and any(not t["executed"] for t in r.trace) and r.success for r in res.values())
    assert any(0 in c.opt.iterations for c in cs)                                                # a zero iteration count
    lines = [str(len(cs))]
    for c in cs:
        lines += case_lines(c)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    exe = compile_driver("depth_odometry_host_driver", pathlib.Path(tempfile.mkdtemp(prefix="depth_odometry_driver_")))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr[-4000:]
