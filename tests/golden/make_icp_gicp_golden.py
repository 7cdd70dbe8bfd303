#!/usr/bin/env python3
"""Generates tests/golden/icp_gicp_golden.npz: the Generalized-ICP restatement (tests/icp_gicp_reference.py) on
BASELINE config 5 (tests/golden/config5_clouds.npz), seeded with the committed TEASER++ pose, r = voxel,
max_iteration = 100, with the covariances of both clouds from the restatement's estimate_covariances at
radius = 2 voxel, max_nn = 20, epsilon = 1e-3.  The covariances are stored as their unit normals (3 doubles per
point, a zero row where fewer than 3 neighbours gave the identity) and rebuilt by the closed formula
C = I - (1 - epsilon) n n^T (icp_gicp_reference.covariances_from_unit_normals), which is how the restatement formed
them: the rebuilt matrices are bit-identical, which compute() asserts.

Asserted here, all at the project's 1e-9 bar, are the decision margins that make an exact comparison legitimate:
over all ICP passes the smallest relative gap between best and second-best d2, the smallest |d2 - r r| / (r r), the
smallest | |d rmse| - relative_rmse | at a stop-rule evaluation; and per point of the covariance estimation the
relative gap between the max_nn-th and (max_nn + 1)-th neighbour d2, the distance of every d2 to radius^2, and the
eigen-gap (lambda1 - lambda0) / lambda2.  Points that fail a neighbourhood margin are listed (source_excluded,
target_excluded) and left out of the covariance comparison; their share may not exceed 1 % of either cloud.
Run from the repo root (CPU only, well under a minute):  python tests/golden/make_icp_gicp_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import icp_reference as R  # noqa: E402
import icp_gicp_reference as RG  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "icp_gicp_golden.npz")
MARGIN = 1e-9
MAX_NN, EPSILON = 20, 1e-3


def cloud_covariances(X, radius):
    C, N, nn_gap, edge, lam = RG.estimate_covariances(X, radius, MAX_NN, EPSILON, details=True)
    with np.errstate(invalid="ignore"):
        eig_gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    bad = (nn_gap < MARGIN) | (edge < MARGIN) | (np.isfinite(eig_gap) & (eig_gap < MARGIN))
    excluded = np.nonzero(bad)[0].astype(np.int32)
    assert len(excluded) <= 0.01 * len(X), (len(excluded), len(X))
    assert np.array_equal(RG.covariances_from_unit_normals(N, EPSILON), C)
    keep = ~bad
    margins = np.array([nn_gap[keep].min(), edge[keep].min(), np.nanmin(eig_gap[keep])])
    return C, N, excluded, margins


def compute():
    P, Q, r, init = R.config5_problem()
    Cs, Ns, ex_s, mg_s = cloud_covariances(P, 2 * r)
    Ct, Nt, ex_t, mg_t = cloud_covariances(Q, 2 * r)
    _, _, fit0, rmse0 = R.corr(R.apply(init, P), Q, r)
    o = RG.registration_icp(P, Q, Cs, Ct, r, init, max_iteration=100, margins=True)
    m = o["margins"]
    for name in ("best_gap", "radius_gap", "stop_gap"):
        assert m[name] >= MARGIN, (name, m[name])
    return dict(source_normals=Ns, target_normals=Nt, source_excluded=ex_s, target_excluded=ex_t,
                source_margins=mg_s, target_margins=mg_t, epsilon=np.float64(EPSILON), max_nn=np.int32(MAX_NN),
                radius=np.float64(2 * r), init=init, r=np.float64(r), max_iteration=np.int32(100),
                init_fitness=np.float64(fit0), init_rmse=np.float64(rmse0), transformation=o["transformation"],
                fitness=np.float64(o["fitness"]), inlier_rmse=np.float64(o["inlier_rmse"]),
                iterations=np.int32(o["iterations"]), correspondence_set=o["correspondence_set"],
                margins=np.array([m["best_gap"], m["radius_gap"], m["stop_gap"]]))


if __name__ == "__main__":
    d = compute()
    np.savez_compressed(OUT, **d)
    print({k: d[k] for k in ("fitness", "inlier_rmse", "iterations", "margins", "source_margins", "target_margins")},
          len(d["correspondence_set"]), "excluded", len(d["source_excluded"]), len(d["target_excluded"]))
    print("seed", d["init_fitness"], d["init_rmse"], "bytes", os.path.getsize(OUT))
