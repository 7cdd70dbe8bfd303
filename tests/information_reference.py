"""numpy restatement of the information-matrix contract (include/teaser_hip.h, "Information matrices").

Open3D's GetInformationMatrixFromPointClouds was restated here, not run: for the pose T and the radius r,
  X = apply(T, P);  C = corr(X)                  (tests/icp_reference.py: the ICP's own apply and corr)
  for (i, j) in C, q = Q[j] as given:  G = [ -[q]x | I3 ],  information = SUM G^T G.
`dtype` is the type the terms are formed and added in (np.float64, or np.longdouble as a yardstick); the correspondences
are always the float64 ones of the contract."""
import numpy as np

import icp_reference as R


def g_matrix(q, dtype=np.float64):
    x, y, z = (dtype(v) for v in q)
    o, l = dtype(0), dtype(1)
    return np.array([[o, z, -y, l, o, o], [-z, o, x, o, l, o], [y, -x, o, o, o, l]], dtype=dtype)


def information(P, Q, r, T, dtype=np.float64):
    """dict(information 6 x 6, abs_terms 6 x 6 = SUM_j |term_j| (the right-hand side of the error bound),
    correspondence_set k x 2 int32, fitness, inlier_rmse)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    j, _, fit, rmse = R.corr(R.apply(np.asarray(T, dtype=np.float64), P), Q, r)
    src = np.nonzero(j >= 0)[0]
    info = np.zeros((6, 6), dtype=dtype)
    mag = np.zeros((6, 6), dtype=dtype)
    for i in src:
        G = g_matrix(Q[j[i]], dtype)
        for a in range(6):  # term by term: a product of three-row columns, each entry rounded on its own
            for b in range(6):
                t = (G[0, a] * G[0, b] + G[1, a] * G[1, b]) + G[2, a] * G[2, b]
                info[a, b] += t
                mag[a, b] += abs(t)
    cs = np.stack([src, j[src]], axis=1).astype(np.int32) if len(src) else np.zeros((0, 2), np.int32)
    return dict(information=info, abs_terms=mag, correspondence_set=cs, fitness=fit, inlier_rmse=rmse)


def information_vectorised(Q, js, dtype=np.float64):
    """SUM G^T G and SUM |G^T G| over the target indices js, entry by entry with array arithmetic (for large sets)."""
    q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)[np.asarray(js, dtype=np.int64)].astype(dtype)
    n = len(q)
    G = np.zeros((n, 3, 6), dtype=dtype)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    G[:, 0, 1], G[:, 0, 2] = z, -y
    G[:, 1, 0], G[:, 1, 2] = -z, x
    G[:, 2, 0], G[:, 2, 1] = y, -x
    G[:, 0, 3] = G[:, 1, 4] = G[:, 2, 5] = 1
    info = np.zeros((6, 6), dtype=dtype)
    mag = np.zeros((6, 6), dtype=dtype)
    for a in range(6):
        for b in range(6):
            t = (G[:, 0, a] * G[:, 0, b] + G[:, 1, a] * G[:, 1, b]) + G[:, 2, a] * G[:, 2, b]
            info[a, b] = t.sum(dtype=dtype) if n else 0
            mag[a, b] = np.abs(t).sum(dtype=dtype) if n else 0
    return info, mag
