#!/usr/bin/env python3
"""Generates tests/golden/icp_step_golden.npz: the cases of tests/icp_step_reference.py (inputs whose arithmetic is
exact in FP64) and, per case, what one ICP step must give, computed from the exact sums at 50 digits and rounded to
FP64: T = U init, the count, fitness and RMSE of the pass, the correspondences, the singular values of H
(point-to-point) or cond(A) (the 6 x 6 solves), H and the two means (for the cases whose R is not unique), and the
error of the project's FP64 restatement against the 50-digit step (the A of the GPU test's bar).
The inputs of the two 65 793-point cases are not stored (icp_step_reference.big_case regenerates them); their
expected results are.  Needs mpmath.  Run from the repo root (CPU only, well under a minute):
  python tests/golden/make_icp_step_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_step_reference as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "icp_step_golden.npz")
INPUTS = ("P", "Q", "init", "N", "Cs", "Ct")
RECORDED = ("T", "cnt", "fitness", "rmse", "match", "exact", "skipped", "sv", "H", "mu_p", "mu_q", "d", "rank", "cond",
            "err_fp64", "keeps")


def compute():
    ctx = S.context()
    d = {}
    names, kinds = [], []
    for c in S.all_reference_cases():
        rec = S.reference(c, ctx)  # asserts exactness, the case's kind and cond <= 1e3 itself
        name = c["name"]
        names.append(name)
        kinds.append(c["kind"])
        d[name + "/meta"] = np.array([c["method"], c["kernel"], int(c["store"])], dtype=np.int64)
        d[name + "/rk"] = np.array([c["r"], c["k"]])
        if c["store"]:
            for key in INPUTS:
                if c[key] is not None:
                    d[name + "/" + key] = np.asarray(c[key], dtype=np.float64)
        for key in RECORDED:
            if key == "match" and not c["store"]:
                assert np.array_equal(rec[key], np.arange(len(c["P"])))  # every source matched to its own target
                continue
            d[name + "/" + key] = rec[key]
    d["names"] = np.array(names)
    d["kinds"] = np.array(kinds)
    return d


if __name__ == "__main__":
    d = compute()
    np.savez_compressed(OUT, **d)
    for name, kind in zip(d["names"], d["kinds"]):
        print("%-20s %-9s count %6d cond %9.3g fp64 restatement error %.3g" % (
            name, kind, d[name + "/cnt"], d[name + "/cond"], d[name + "/err_fp64"]))
    print("bytes", os.path.getsize(OUT))
