#!/usr/bin/env python3
"""Generates tests/golden/icp_plane_golden.npz: the point-to-plane ICP restatement (tests/icp_plane_reference.py) on
BASELINE config 5 (tests/golden/config5_clouds.npz), seeded with the committed TEASER++ pose, r = voxel,
max_iteration = 100, for the L2 kernel and for Tukey with k = voxel / 2.  The target normals come from the features
oracle (oracle/features.py: estimate_normals(Q, 2 * voxel), the radius make_config5_result_golden.py uses), rows that
are not finite (PCL gives NaN below 3 neighbours) set to zero, stored as float64.

Also recorded, and asserted here, are the decision margins that make an exact comparison of correspondence sets and
iteration counts legitimate: over all passes the smallest relative gap between a source point's best and second-best
d2, the smallest |d2 - r r| / (r r), and the smallest | |d rmse| - relative_rmse | at a stop-rule evaluation.  Each
must be >= 1e-9, a thousand times the 1e-12 agreement the suite holds fitness and RMSE to.
Run from the repo root (CPU only, well under a minute):  python tests/golden/make_icp_plane_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import icp_reference as R  # noqa: E402
import icp_plane_reference as RP  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "icp_plane_golden.npz")
MARGIN = 1e-9
KERNELS = (("l2", 1.0), ("tukey", 0.5))  # (kernel, k in voxels)


def target_normals(Q, voxel):
    from oracle import features as F
    nv = F.estimate_normals(Q, 2 * voxel).astype(np.float64)
    nv[~np.isfinite(nv).all(axis=1)] = 0.0
    return nv


def compute():
    P, Q, r, init = R.config5_problem()
    N = target_normals(Q, r)
    _, _, fit0, rmse0 = R.corr(R.apply(init, P), Q, r)
    d = dict(target_normals=N, init=init, r=np.float64(r), max_iteration=np.int32(100),
             init_fitness=np.float64(fit0), init_rmse=np.float64(rmse0))
    for kernel, kv in KERNELS:
        k = kv * r
        o = RP.registration_icp(P, Q, N, r, init, kernel=kernel, k=k, max_iteration=100, margins=True)
        m = o["margins"]
        for name in ("best_gap", "radius_gap", "stop_gap"):
            assert m[name] >= MARGIN, (kernel, name, m[name])
        d.update({kernel + "_transformation": o["transformation"], kernel + "_fitness": np.float64(o["fitness"]),
                  kernel + "_inlier_rmse": np.float64(o["inlier_rmse"]),
                  kernel + "_iterations": np.int32(o["iterations"]),
                  kernel + "_correspondence_set": o["correspondence_set"], kernel + "_k": np.float64(k),
                  kernel + "_margins": np.array([m["best_gap"], m["radius_gap"], m["stop_gap"]])})
    return d


if __name__ == "__main__":
    d = compute()
    np.savez_compressed(OUT, **d)
    for kernel, _ in KERNELS:
        print(kernel, {k: d[kernel + "_" + k] for k in ("fitness", "inlier_rmse", "iterations", "margins")},
              len(d[kernel + "_correspondence_set"]))
    print("seed", d["init_fitness"], d["init_rmse"], "bytes", os.path.getsize(OUT))
