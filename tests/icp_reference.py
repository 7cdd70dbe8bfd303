"""numpy restatement of the point-to-point ICP contract (include/teaser_hip.h, "ICP refinement").

Open3D's RegistrationICP with TransformationEstimationPointToPoint(with_scaling=False), written out step by step:
  apply(T, p)_row = ((T[row,0] x + T[row,1] y) + T[row,2] z) + T[row,3]          (no fused operations)
  corr(X): for each source point i the lexicographic minimum of (d2, j) over the targets with
           d2 = ((dx dx + dy dy) + dz dz) < r r, dx = X.x - Q.x  (strict: a point at exactly r is not a match)
  loop:    X = apply(init, P), T = init, res = corr(X); for it = 1..max_iteration: U = umeyama(X[C.src], Q[C.dst])
           (identity when C is empty), T = U T, X = apply(U, X), prev = res, res = corr(X), stop when
           |prev.fitness - res.fitness| < relative_fitness and |prev.rmse - res.rmse| < relative_rmse
           (ABSOLUTE differences, despite the names).
Candidates come from scipy's cKDTree at a radius slightly above r; d2 is then recomputed with the exact expression
and the strict test applied, so the tree's own rounding cannot change the result."""
import numpy as np
from scipy.spatial import cKDTree


def apply(T, X):
    T = np.asarray(T, dtype=np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    out = np.empty_like(X)
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def compose(U, T):
    """U T, each entry ((U[r,0] T[0,c] + U[r,1] T[1,c]) + U[r,2] T[2,c]) + U[r,3] T[3,c]."""
    out = np.empty((4, 4))
    for r in range(4):
        for c in range(4):
            out[r, c] = ((U[r, 0] * T[0, c] + U[r, 1] * T[1, c]) + U[r, 2] * T[2, c]) + U[r, 3] * T[3, c]
    return out


def corr(X, Q, r, tree=None):
    """(match index per source point or -1, d2 per source point, fitness, inlier_rmse)."""
    n_s = len(X)
    j_best = np.full(n_s, -1, dtype=np.int64)
    d_best = np.zeros(n_s)
    if n_s and len(Q):
        tree = tree if tree is not None else cKDTree(Q)
        cands = tree.query_ball_point(X, r * (1 + 1e-9))
        r2 = r * r
        for i, js in enumerate(cands):
            if not js:
                continue
            js = np.asarray(js, dtype=np.int64)
            dx = X[i, 0] - Q[js, 0]
            dy = X[i, 1] - Q[js, 1]
            dz = X[i, 2] - Q[js, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            keep = d2 < r2
            if not keep.any():
                continue
            js, d2 = js[keep], d2[keep]
            k = np.lexsort((js, d2))[0]
            j_best[i], d_best[i] = js[k], d2[k]
    m = j_best >= 0
    cnt = int(m.sum())
    fitness = cnt / n_s if n_s and cnt else 0.0
    rmse = float(np.sqrt(d_best[m].sum() / cnt)) if cnt else 0.0
    return j_best, d_best, fitness, rmse


def umeyama(P, Q):
    """Rigid (no scaling) least-squares transform P -> Q as a 4x4: R = V diag(1,1,s) U^T from the SVD
    H = U S V^T of the two-pass centred cross-covariance H = sum (p - mu_P)(q - mu_Q)^T, s = -1 iff
    det(U) det(V) < 0, t = mu_Q - R mu_P."""
    out = np.eye(4)
    if len(P) == 0:
        return out
    mp, mq = P.mean(axis=0), Q.mean(axis=0)
    H = (P - mp).T @ (Q - mq)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(V) < 0:
        D[2, 2] = -1
    R = V @ D @ U.T
    out[:3, :3] = R
    out[:3, 3] = mq - R @ mp
    return out


def registration_icp(source, target, r, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """Returns dict(transformation, fitness, inlier_rmse, correspondence_set (k x 2, sorted by source), iterations)."""
    P = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    tree = cKDTree(Q) if len(Q) else None
    X = apply(T, P)
    j, d2, fit, rmse = corr(X, Q, r, tree)
    it = 0
    while it < max_iteration:
        it += 1
        m = j >= 0
        U = umeyama(X[m], Q[j[m]])
        T = compose(U, T)
        X = apply(U, X)
        pf, pr = fit, rmse
        j, d2, fit, rmse = corr(X, Q, r, tree)
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    src = np.nonzero(j >= 0)[0]
    cs = np.stack([src, j[src]], axis=1).astype(np.int32) if len(src) else np.zeros((0, 2), np.int32)
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, correspondence_set=cs, iterations=it)


def config5_problem():
    """The config-5 pair (tests/golden/config5_clouds.npz) and the committed TEASER++ pose as the ICP seed."""
    import json
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    c5 = np.load(os.path.join(here, "golden", "config5_clouds.npz"))
    g = json.load(open(os.path.join(here, "golden", "config5_result_golden.json")))
    init = np.eye(4)
    init[:3, :3] = np.asarray(g["rotation"]).reshape(3, 3)
    init[:3, 3] = g["translation"]
    return (c5["cloud_bin_0"].astype(np.float64), c5["cloud_bin_4"].astype(np.float64), float(c5["voxel_size"]),
            init)
