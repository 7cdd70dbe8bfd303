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


# ---- the inputs the tests share ----
def grid_pair(seed, n_s, n_t):
    """Integer clouds in [-64, 64] and a pose (signed axis permutation + integer shift) under which the first
    ceil(2 n_s / 3) source points land exactly on target points (duplicates among the targets included, so ties
    occur) and the others a whole unit or more away from every target."""
    rng = np.random.default_rng(seed)
    T = np.zeros((4, 4))
    T[0, 2], T[1, 0], T[2, 1], T[3, 3] = -1.0, 1.0, -1.0, 1.0
    T[:3, 3] = [3.0, -7.0, 11.0]
    Q = rng.integers(-12, 13, size=(n_t, 3)).astype(np.float64) * np.array([5.0, 4.0, 2.0])  # |coordinates| <= 60
    X = np.zeros((n_s, 3))
    hit = (2 * n_s + 2) // 3
    if n_t:
        X[:hit] = Q[rng.integers(0, n_t, size=hit)]
        X[hit:] = Q[rng.integers(0, n_t, size=n_s - hit)] + np.array([1.0, 1.0, 1.0])  # off the 5 x 4 x 2 lattice
    P = (X - T[:3, 3]) @ T[:3, :3]  # T^-1 X, exact
    assert np.array_equal(R.apply(T, P), X)
    return P, Q, T


K_ICP_BLOCK = 256  # kIcpBlock of csrc/icp_internal.h: source points per block of the packed batch
WIDE_BATCH = 320
WIDE_FAR = 138  # the problem of the wide batch whose pose moves every source point away from every target


def wide_batch():
    """320 integer-grid problems (bit-equal to numpy: every product and sum is exact) whose source sizes cycle 0, 1,
    kIcpBlock - 1, kIcpBlock, kIcpBlock + 1 and whose targets have 300, 60, 1 or 0 points: a list of (P, Q, T, r).
    Problem WIDE_FAR's pose is shifted by 1000 units, so no point lies within r.  What the wide test rests on is
    asserted from the sizes alone."""
    b = WIDE_BATCH
    sizes = (0, 1, K_ICP_BLOCK - 1, K_ICP_BLOCK, K_ICP_BLOCK + 1)
    n_s = [sizes[i % len(sizes)] for i in range(b)]
    n_t = [0 if i % 7 == 3 else (300, 60, 1)[i % 3] for i in range(b)]
    assert b > 256  # icp_info_finalize_kernel: a workgroup per problem
    assert sum((k + K_ICP_BLOCK - 1) // K_ICP_BLOCK for k in n_s) > 256  # icp_info_block_kernel: blk_prob past 256 entries
    assert n_s[WIDE_FAR] >= K_ICP_BLOCK and n_t[WIDE_FAR] == 300
    assert len({n_s[255], n_s[256], n_s[257]}) == 3 and n_s[b - 1] > 0
    out = []
    for i in range(b):
        P, Q, T = grid_pair(600 + i, n_s[i], n_t[i])
        if i == WIDE_FAR:
            T = T.copy()
            T[:3, 3] += 1000.0
        out.append((P, Q, T, 0.5))
    return out
