"""Writes tests/golden/fgr_golden.npz: the shapes of tests/fgr_reference.py (CASES) with their inputs and the
per-iteration records of the restatement in np.longdouble, each longdouble array stored as two float64 arrays
(NAME_hi + NAME_lo), beside the float64 restatement's pose and its distance from the longdouble one -- the measured
figure the GPU test's end-to-end bar is a multiple of.

    python tests/golden/make_fgr_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fgr_reference as ref  # noqa: E402


def split(a):
    a = np.asarray(a, dtype=np.longdouble)
    hi = a.astype(np.float64)
    return hi, (a - hi).astype(np.float64)


def main():
    out = {}
    for name in ref.CASES:
        P, Q, corr, T_true, opt = ref.case(name)
        ld = ref.fgr(P, Q, corr, dtype=np.longdouble, **opt)
        f64 = ref.fgr(P, Q, corr, dtype=np.float64, **opt)
        out[name + "/P"], out[name + "/Q"], out[name + "/corr"], out[name + "/T_true"] = P, Q, corr, T_true
        for key in ("transformation", "optimised", "mu", "xi", "trans", "mean_p", "mean_q", "scale", "final_mu"):
            out[name + "/" + key + "_hi"], out[name + "/" + key + "_lo"] = split(ld[key])
        out[name + "/counts"] = np.array([ld["iterations"], ld["failed_solves"], ld["flags"]], dtype=np.int32)
        out[name + "/T_f64"] = f64["transformation"]
        d = float(np.abs(f64["transformation"].astype(np.longdouble) - ld["transformation"]).max())
        out[name + "/distance_f64"] = np.array(d)
        print("%-9s ncorr %5d iterations %2d failed %d  |T_f64 - T_ld| %.3g  |T_ld - T_true| %.3g" % (
            name, len(corr), ld["iterations"], ld["failed_solves"], d,
            float(np.abs(ld["transformation"] - T_true).max())))
    path = os.path.join(HERE, "fgr_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
