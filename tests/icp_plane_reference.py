"""numpy restatement of the point-to-plane ICP contract (include/teaser_hip.h, "ICP refinement: point-to-plane";
DESIGN.md section 12).  apply, compose and corr -- the loop, the search, fitness, the Euclidean inlier RMSE and the
stop rule -- are those of the point-to-point restatement (tests/icp_reference.py); only the step U differs:

  c = the target's bounding-box centre; per correspondence (i, j): x' = x - c, q' = q - c, e = x' - q',
  r = (e0 n0 + e1 n1) + e2 n2,  w = kernel(r),  J = [x' x n ; n],  A = sum w J J^T,  g = sum w r J
  (ascending source order), A xi = -g by LDL^T without pivoting, R = Rz(gamma) Ry(beta) Rx(alpha),
  U = [R | t' + c - R c]; U = identity when C is empty, a pivot is not finite or not positive, or xi is not finite."""
import numpy as np
from scipy.spatial import cKDTree

from icp_reference import apply, compose, corr

KERNELS = ("l2", "huber", "cauchy", "gm", "tukey")


def weight(kernel, k, r):
    """Open3D's RobustKernel::Weight(r) for the five kernels of the contract; r may be an array."""
    r = np.asarray(r, dtype=np.float64)
    if kernel == "l2":
        return np.ones_like(r)
    a = np.abs(r)
    if kernel == "huber":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(a <= k, 1.0, k / a)
    if kernel == "cauchy":
        q = r / k
        return 1.0 / (1.0 + q * q)
    if kernel == "gm":
        s = k + r * r
        return k / (s * s)
    if kernel == "tukey":
        q = r / k
        u = 1.0 - q * q
        return np.where(a <= k, u * u, 0.0)
    raise ValueError("unknown kernel %r" % (kernel,))


def centre_of(Q):
    """The point the sums are centred on: the target's bounding-box centre (0 for an empty target)."""
    if len(Q) == 0:
        return np.zeros(3)
    return 0.5 * (Q.min(axis=0) + Q.max(axis=0))


def normal_equations(X, Q, N, c, kernel="l2", k=1.0, order=None, chunk=None):
    """(A, g) of the matched rows X, Q, N (m x 3 each).  order: a permutation of the rows to sum in (default
    ascending); chunk: sum in chunks of that many rows first, then the chunk sums in order (the GPU's shape)."""
    xp, qp = X - c, Q - c
    e = xp - qp
    r = (e[:, 0] * N[:, 0] + e[:, 1] * N[:, 1]) + e[:, 2] * N[:, 2]
    w = weight(kernel, k, r)
    J = np.empty((len(X), 6))
    J[:, 0] = xp[:, 1] * N[:, 2] - xp[:, 2] * N[:, 1]
    J[:, 1] = xp[:, 2] * N[:, 0] - xp[:, 0] * N[:, 2]
    J[:, 2] = xp[:, 0] * N[:, 1] - xp[:, 1] * N[:, 0]
    J[:, 3:] = N
    if order is not None:
        J, w, r = J[order], w[order], r[order]
    terms_A = (w[:, None] * J)[:, :, None] * J[:, None, :]
    terms_g = (w * r)[:, None] * J

    def seq(t):  # strictly sequential sum over the first axis
        return np.cumsum(t, axis=0)[-1] if len(t) else np.zeros(t.shape[1:])

    if chunk:
        parts_A = [seq(terms_A[s:s + chunk]) for s in range(0, len(J), chunk)]
        parts_g = [seq(terms_g[s:s + chunk]) for s in range(0, len(J), chunk)]
        return seq(np.array(parts_A).reshape(-1, 6, 6)), seq(np.array(parts_g).reshape(-1, 6))
    return seq(terms_A), seq(terms_g)


def solve6(A, g):
    """xi with A xi = -g by LDL^T without pivoting, or None when a pivot is not finite or not positive or xi is not
    finite."""
    L = np.eye(6)
    d = np.zeros(6)
    for j in range(6):
        s = A[j, j]
        for k in range(j):
            s -= L[j, k] * L[j, k] * d[k]
        if not np.isfinite(s) or not s > 0:
            return None
        d[j] = s
        for i in range(j + 1, 6):
            t = A[i, j]
            for k in range(j):
                t -= L[i, k] * L[j, k] * d[k]
            L[i, j] = t / s
    y = np.zeros(6)
    for i in range(6):
        t = -g[i]
        for k in range(i):
            t -= L[i, k] * y[k]
        y[i] = t
    y = y / d
    xi = np.zeros(6)
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t -= L[k, i] * xi[k]
        xi[i] = t
    return xi if np.isfinite(xi).all() else None


def step_matrix(xi, c):
    """U = [R | t' + c - R c], R = Rz(gamma) Ry(beta) Rx(alpha) (Open3D's TransformVector6dToMatrix4d)."""
    ca, sa, cb, sb, cg, sg = np.cos(xi[0]), np.sin(xi[0]), np.cos(xi[1]), np.sin(xi[1]), np.cos(xi[2]), np.sin(xi[2])
    Rm = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                   [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                   [-sb, cb * sa, cb * ca]])
    U = np.eye(4)
    U[:3, :3] = Rm
    for r in range(3):
        U[r, 3] = (xi[3 + r] + c[r]) - ((Rm[r, 0] * c[0] + Rm[r, 1] * c[1]) + Rm[r, 2] * c[2])
    return U


def plane_step(X, Q, N, c, kernel="l2", k=1.0, order=None, chunk=None):
    if len(X) == 0:
        return np.eye(4)
    A, g = normal_equations(X, Q, N, c, kernel, k, order, chunk)
    xi = solve6(A, g)
    return np.eye(4) if xi is None else step_matrix(xi, c)


def margins_of(X, Q, r, tree):
    """Decision margins of one correspondence pass: the smallest relative gap between a source point's best and
    second-best d2 among the targets inside r, and the smallest |d2 - r r| / (r r) over every pair near the radius."""
    gap, edge = np.inf, np.inf
    if len(X) == 0 or len(Q) == 0:
        return gap, edge
    r2 = r * r
    for i, js in enumerate(tree.query_ball_point(X, r * 1.01)):
        if not js:
            continue
        js = np.asarray(js, dtype=np.int64)
        dx, dy, dz = X[i, 0] - Q[js, 0], X[i, 1] - Q[js, 1], X[i, 2] - Q[js, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        edge = min(edge, float(np.abs(d2 - r2).min() / r2))
        inside = np.sort(d2[d2 < r2])
        if len(inside) >= 2:
            gap = min(gap, float((inside[1] - inside[0]) / inside[1]) if inside[1] > 0 else 0.0)
    return gap, edge


def registration_icp(source, target, target_normals, r, init=None, kernel="l2", k=1.0, max_iteration=30,
                     relative_fitness=1e-6, relative_rmse=1e-6, margins=False, order_seed=None, chunk=None):
    """Returns dict(transformation, fitness, inlier_rmse, correspondence_set (k x 2, sorted by source), iterations).
    margins=True adds dict 'margins' (best_gap, radius_gap, stop_gap: the smallest over all passes / stop-rule
    evaluations).  order_seed / chunk: sum A and g in a shuffled order / in chunks (to measure the sensitivity)."""
    P = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    N = np.asarray(target_normals, dtype=np.float64).reshape(-1, 3)
    assert N.shape == Q.shape
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
        order = rng.permutation(int(m.sum())) if rng is not None else None
        U = plane_step(X[m], Q[j[m]], N[j[m]], c, kernel, k, order, chunk)
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


def config5_normals():
    """Target normals of the config-5 pair as the committed fixture holds them (float64, NaN rows zeroed)."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, "golden", "icp_plane_golden.npz"))["target_normals"]
