"""numpy restatement of the Generalized-ICP contract and of the covariance estimation that goes with it
(include/teaser_hip.h, "ICP refinement: Generalized ICP" and "Covariance estimation").
apply, compose and corr -- the loop, the search, fitness, the Euclidean inlier RMSE and the stop rule -- are those of
the point-to-point restatement (tests/icp_reference.py); the 6 x 6 solve and the step matrix are those of the
point-to-plane restatement (tests/icp_plane_reference.py).  Only what a correspondence adds to A and g differs:

  c = the target's bounding-box centre, Rk = the rotation block of the accumulated T; per correspondence (i, j):
  x' = x - c, q' = q - c, e = x' - q', M = Ct[j] + Rk Cs[i] Rk^T, W = adj(M) / det(M) (nothing added when det is not
  finite or not > 0), J = [-[x']x | I], A = sum J^T W J, g = sum J^T W e, summed one correspondence at a time in
  ascending source order.

Covariances: per point the (at most max_nn) smallest (d2, j) with d2 < radius^2, sums of the offsets and their outer
products in that order, a cyclic Jacobi iteration, C = I - (1 - eps) n n^T."""
import numpy as np
from scipy.spatial import cKDTree

from icp_plane_reference import centre_of, solve6, step_matrix
from icp_reference import apply, compose, corr

UPPER = (0, 1, 2, 4, 5, 8)


def sym_upper(C):
    """n x 3 x 3 (or n x 9) -> the six entries the contract reads, n x 6: 00 01 02 11 12 22."""
    return np.asarray(C, dtype=np.float64).reshape(-1, 9)[:, UPPER]


def information(Cs6, Ct6, Rk):
    """W (n x 6, upper triangle) and the mask of the correspondences that contribute, from the packed covariances of
    the matched rows."""
    S = Cs6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    B = np.empty_like(S)
    for r in range(3):
        for c in range(3):
            B[:, r, c] = (Rk[r, 0] * S[:, 0, c] + Rk[r, 1] * S[:, 1, c]) + Rk[r, 2] * S[:, 2, c]

    def rcr(r, c):
        return (B[:, r, 0] * Rk[c, 0] + B[:, r, 1] * Rk[c, 1]) + B[:, r, 2] * Rk[c, 2]

    m00, m01, m02 = Ct6[:, 0] + rcr(0, 0), Ct6[:, 1] + rcr(0, 1), Ct6[:, 2] + rcr(0, 2)
    m11, m12, m22 = Ct6[:, 3] + rcr(1, 1), Ct6[:, 4] + rcr(1, 2), Ct6[:, 5] + rcr(2, 2)
    a00, a01, a02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
    a11, a12, a22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    det = (m00 * a00 + m01 * a01) + m02 * a02
    ok = np.isfinite(det) & (det > 0)
    with np.errstate(all="ignore"):
        W = np.stack([a00, a01, a02, a11, a12, a22], 1) / det[:, None]
    return W, ok


def terms_from_W(xp, e, W6):
    """What each correspondence adds: (n x 6 x 6 symmetric, n x 6) from x', e and the upper triangle of W."""
    n = len(xp)
    W = W6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(n, 3, 3)
    x0, x1, x2 = xp[:, 0], xp[:, 1], xp[:, 2]
    we = np.empty((n, 3))
    for r in range(3):
        we[:, r] = (W[:, r, 0] * e[:, 0] + W[:, r, 1] * e[:, 1]) + W[:, r, 2] * e[:, 2]
    G = np.empty((n, 3, 3))  # [x']x W: column k = x' x column k of W
    for k in range(3):
        G[:, 0, k] = x1 * W[:, 2, k] - x2 * W[:, 1, k]
        G[:, 1, k] = x2 * W[:, 0, k] - x0 * W[:, 2, k]
        G[:, 2, k] = x0 * W[:, 1, k] - x1 * W[:, 0, k]
    A = np.zeros((n, 6, 6))
    for r in range(3):  # row r of the rotation block = x' x row r of G
        A[:, r, 0] = x1 * G[:, r, 2] - x2 * G[:, r, 1]
        A[:, r, 1] = x2 * G[:, r, 0] - x0 * G[:, r, 2]
        A[:, r, 2] = x0 * G[:, r, 1] - x1 * G[:, r, 0]
    A[:, :3, 3:] = G
    A[:, 3:, 3:] = W
    iu = np.triu_indices(6)
    U = np.zeros_like(A)
    U[:, iu[0], iu[1]] = A[:, iu[0], iu[1]]  # the contract sums the upper triangle; mirror it
    A = U + np.transpose(np.triu(U, 1), (0, 2, 1))
    g = np.empty((n, 6))
    g[:, 0] = x1 * we[:, 2] - x2 * we[:, 1]
    g[:, 1] = x2 * we[:, 0] - x0 * we[:, 2]
    g[:, 2] = x0 * we[:, 1] - x1 * we[:, 0]
    g[:, 3:] = we
    return A, g


def _seq(t):
    return np.cumsum(t, axis=0)[-1] if len(t) else np.zeros(t.shape[1:])


def sum_terms(tA, tg, order=None, chunk=None):
    """Strictly sequential sums; order: a permutation to sum in; chunk: chunks of that many rows first (the GPU's
    shape: 256 source points per block, blocks in order)."""
    if order is not None:
        tA, tg = tA[order], tg[order]
    if chunk:
        pa = [_seq(tA[s:s + chunk]) for s in range(0, len(tA), chunk)]
        pg = [_seq(tg[s:s + chunk]) for s in range(0, len(tg), chunk)]
        return _seq(np.array(pa).reshape(-1, 6, 6)), _seq(np.array(pg).reshape(-1, 6))
    return _seq(tA), _seq(tg)


def normal_equations(X, Q, Cs6, Ct6, Rk, c, order=None, chunk=None):
    """(A, g) of the matched rows (X, Q m x 3; Cs6, Ct6 m x 6)."""
    xp, qp = X - c, Q - c
    e = xp - qp
    W, ok = information(Cs6, Ct6, Rk)
    tA, tg = terms_from_W(xp[ok], e[ok], W[ok])
    full_A, full_g = np.zeros((len(X), 6, 6)), np.zeros((len(X), 6))
    full_A[ok], full_g[ok] = tA, tg  # a left-out correspondence adds zeros: the sum's order is untouched
    return sum_terms(full_A, full_g, order, chunk)


def gicp_step(X, Q, Cs6, Ct6, Rk, c, order=None, chunk=None):
    if len(X) == 0:
        return np.eye(4)
    A, g = normal_equations(X, Q, Cs6, Ct6, Rk, c, order, chunk)
    xi = solve6(A, g)
    return np.eye(4) if xi is None else step_matrix(xi, c)


def registration_icp(source, target, source_cov, target_cov, r, init=None, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, margins=False, order_seed=None, chunk=None):
    """Returns dict(transformation, fitness, inlier_rmse, correspondence_set, iterations) (+ 'margins' as
    icp_plane_reference.registration_icp does).  order_seed / chunk: sum A and g in a shuffled order / in chunks."""
    from icp_plane_reference import margins_of
    P = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    Cs6, Ct6 = sym_upper(source_cov), sym_upper(target_cov)
    assert len(Cs6) == len(P) and len(Ct6) == len(Q)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    c = centre_of(Q)
    tree = cKDTree(Q) if len(Q) else None
    rng = np.random.default_rng(order_seed) if order_seed is not None else None
    X = apply(T, P)
    j, d2, fit, rmse = corr(X, Q, r, tree)
    mg = dict(best_gap=np.inf, radius_gap=np.inf, stop_gap=np.inf)

    def note():
        if margins:
            a, b = margins_of(X, Q, r, tree)
            mg["best_gap"], mg["radius_gap"] = min(mg["best_gap"], a), min(mg["radius_gap"], b)

    note()
    it = 0
    while it < max_iteration:
        it += 1
        m = j >= 0
        if chunk:  # the GPU's blocks hold 256 SOURCE points, matched or not
            U = _chunked_step(X, Q, Cs6, Ct6, T[:3, :3], c, j, chunk)
        else:
            order = rng.permutation(int(m.sum())) if rng is not None else None
            U = gicp_step(X[m], Q[j[m]], Cs6[m], Ct6[j[m]], T[:3, :3], c, order)
        T = compose(U, T)
        X = apply(U, X)
        pf, pr = fit, rmse
        j, d2, fit, rmse = corr(X, Q, r, tree)
        note()
        mg["stop_gap"] = min(mg["stop_gap"], abs(abs(pr - rmse) - relative_rmse))
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    src = np.nonzero(j >= 0)[0]
    cs = np.stack([src, j[src]], axis=1).astype(np.int32) if len(src) else np.zeros((0, 2), np.int32)
    out = dict(transformation=T, fitness=fit, inlier_rmse=rmse, correspondence_set=cs, iterations=it)
    if margins:
        out["margins"] = mg
    return out


def _chunked_step(X, Q, Cs6, Ct6, Rk, c, j, chunk):
    """The step with the sums taken per chunk of `chunk` consecutive source points, then over the chunks."""
    m = j >= 0
    if not m.any():
        return np.eye(4)
    xp, qp = X[m] - c, Q[j[m]] - c
    W, ok = information(Cs6[m], Ct6[j[m]], Rk)
    tA, tg = np.zeros((int(m.sum()), 6, 6)), np.zeros((int(m.sum()), 6))
    tA[ok], tg[ok] = terms_from_W(xp[ok], (xp - qp)[ok], W[ok])
    blk = np.nonzero(m)[0] // chunk
    pa = [_seq(tA[blk == b]) for b in np.unique(blk)]
    pg = [_seq(tg[blk == b]) for b in np.unique(blk)]
    xi = solve6(_seq(np.array(pa)), _seq(np.array(pg)))
    return np.eye(4) if xi is None else step_matrix(xi, c)


# ---- covariance estimation ------------------------------------------------------------------------------------------
def neighbourhood(P, i, radius, max_nn, tree):
    """(indices in ascending (d2, j), their d2, the d2 of the first neighbour left out by max_nn or None)."""
    js = np.asarray(tree.query_ball_point(P[i], radius * (1 + 1e-9)), dtype=np.int64)
    dx, dy, dz = P[i, 0] - P[js, 0], P[i, 1] - P[js, 1], P[i, 2] - P[js, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    keep = d2 < radius * radius
    js, d2 = js[keep], d2[keep]
    o = np.lexsort((js, d2))
    js, d2 = js[o], d2[o]
    nxt = float(d2[max_nn]) if len(js) > max_nn else None
    return js[:max_nn], d2[:max_nn], nxt


def sample_covariance(P, i, js):
    """The six upper entries (00 01 02 11 12 22), sums added one neighbour at a time in the given order."""
    o = P[js] - P[i]
    m = len(js)
    s1 = _seq(o)
    prod = np.stack([o[:, 0] * o[:, 0], o[:, 0] * o[:, 1], o[:, 0] * o[:, 2], o[:, 1] * o[:, 1], o[:, 1] * o[:, 2],
                     o[:, 2] * o[:, 2]], 1)
    s2 = _seq(prod)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    return np.array([(s2[k] - (s1[a] * s1[b]) / m) / (m - 1) for k, (a, b) in enumerate(pairs)])


def jacobi3(a6):
    """The contract's cyclic Jacobi: (diagonal, V) of the symmetric 3 x 3 given by its upper triangle."""
    A = np.array([[a6[0], a6[1], a6[2]], [a6[1], a6[3], a6[4]], [a6[2], a6[4], a6[5]]], dtype=np.float64)
    V = np.eye(3)
    for _ in range(16):
        rotated = False
        for p, q, o in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq, app, aqq = A[p, q], A[p, p], A[q, q]
            if apq == 0.0 or abs(apq) <= 1e-17 * (abs(app) + abs(aqq)):
                continue
            rotated = True
            theta = (aqq - app) / (2.0 * apq)
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(1.0 + theta * theta))
            cs = 1.0 / np.sqrt(1.0 + t * t)
            sn = t * cs
            A[p, p], A[q, q] = app - t * apq, aqq + t * apq
            A[p, q] = A[q, p] = 0.0
            aop, aoq = A[o, p], A[o, q]
            A[o, p] = A[p, o] = cs * aop - sn * aoq
            A[o, q] = A[q, o] = sn * aop + cs * aoq
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = cs * vp - sn * vq, sn * vp + cs * vq
        if not rotated:
            break
    return np.diag(A).copy(), V


def covariance_from_unit_normal(n, eps):
    u = (1.0 - eps) * n
    C = np.eye(3)
    for a in range(3):
        for b in range(3):
            C[a, b] = (1.0 if a == b else 0.0) - u[min(a, b)] * n[max(a, b)]
    return C


def estimate_covariances(points, radius, max_nn=20, epsilon=1e-3, details=False):
    """n x 3 x 3 covariances; details=True adds (normals n x 3 (zero where the identity was given), the relative gap
    between the max_nn-th and (max_nn + 1)-th d2 per point (inf when max_nn does not bind), the relative distance of
    the nearest d2 to radius^2 per point, the eigenvalues in ascending order per point (nan below 3 neighbours))."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    C = np.tile(np.eye(3), (n, 1, 1))
    N = np.zeros((n, 3))
    nn_gap, edge, lam = np.full(n, np.inf), np.full(n, np.inf), np.full((n, 3), np.nan)
    if n == 0:
        return (C, N, nn_gap, edge, lam) if details else C
    tree = cKDTree(P)
    r2 = radius * radius
    for i in range(n):
        js, d2, nxt = neighbourhood(P, i, radius, max_nn, tree)
        if details:
            near = np.asarray(tree.query_ball_point(P[i], radius * 1.01), dtype=np.int64)
            ex, ey, ez = P[i, 0] - P[near, 0], P[i, 1] - P[near, 1], P[i, 2] - P[near, 2]
            edge[i] = np.abs(((ex * ex + ey * ey) + ez * ez) - r2).min() / r2
            if nxt is not None:
                nn_gap[i] = (nxt - d2[-1]) / nxt if nxt > 0 else 0.0
        if len(js) < 3:
            continue
        diag, V = jacobi3(sample_covariance(P, i, js))
        k = 0
        if diag[1] < diag[k]:
            k = 1
        if diag[2] < diag[k]:
            k = 2
        v = V[:, k]
        v = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        N[i] = v
        lam[i] = np.sort(diag)
        C[i] = covariance_from_unit_normal(v, epsilon)
    return (C, N, nn_gap, edge, lam) if details else C


def covariances_from_normals(normals, epsilon=1e-3):
    """I - (1 - eps) n n^T / (n^T n); the identity for a zero or non-finite normal."""
    N = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    C = np.tile(np.eye(3), (len(N), 1, 1))
    for i, v in enumerate(N):
        with np.errstate(all="ignore"):
            nn = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if np.isfinite(v).all() and np.isfinite(nn) and nn > 0:
            C[i] = np.eye(3) - ((1.0 - epsilon) * v)[:, None] * v[None, :] / nn
    return C


def covariances_from_unit_normals(N, epsilon=1e-3):
    """What estimate_covariances returned, rebuilt from its unit normals (a zero row: the identity) by the closed
    formula of the contract -- the form the committed fixture stores."""
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    C = np.tile(np.eye(3), (len(N), 1, 1))
    for i, v in enumerate(N):
        if v.any():
            C[i] = covariance_from_unit_normal(v, epsilon)
    return C


def config5_covariances():
    """(Cs, Ct) of the config-5 pair as the committed fixture holds them."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", "icp_gicp_golden.npz"))
    eps = float(g["epsilon"])
    return covariances_from_unit_normals(g["source_normals"], eps), covariances_from_unit_normals(g["target_normals"], eps)
