#!/usr/bin/env python3
"""Generates tests/golden/icp_golden.npz: the ICP restatement (tests/icp_reference.py) on BASELINE config 5 (the
3DMatch pair of tests/golden/config5_clouds.npz), seeded with the committed TEASER++ pose of
tests/golden/config5_result_golden.json, r = voxel, max_iteration = 100 (the tutorial's refinement step).
Recorded: T, fitness, inlier_rmse, iterations, the correspondence set, and the fitness / rmse of the seed pose.
Run from the repo root (CPU only, a few seconds):  python tests/golden/make_icp_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "icp_golden.npz")


def compute():
    P, Q, r, init = R.config5_problem()
    _, _, fit0, rmse0 = R.corr(R.apply(init, P), Q, r)
    o = R.registration_icp(P, Q, r, init, max_iteration=100)
    return dict(transformation=o["transformation"], fitness=np.float64(o["fitness"]),
                inlier_rmse=np.float64(o["inlier_rmse"]), iterations=np.int32(o["iterations"]),
                correspondence_set=o["correspondence_set"], init=init, r=np.float64(r), max_iteration=np.int32(100),
                init_fitness=np.float64(fit0), init_rmse=np.float64(rmse0))


if __name__ == "__main__":
    d = compute()
    np.savez_compressed(OUT, **d)
    print({k: d[k] for k in ("fitness", "inlier_rmse", "iterations", "init_fitness", "init_rmse")},
          len(d["correspondence_set"]))
