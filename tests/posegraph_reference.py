"""numpy restatement of pose-graph optimisation in Open3D's formulation (PoseGraph, global_optimization with
GlobalOptimizationLevenbergMarquardt: Levenberg-Marquardt with a line process on the uncertain edges, then edge
pruning).  Open3D was restated here, not run.  The library has no pose-graph optimiser yet; this file is the parity
target a device implementation is to be tested against, and it consumes the information matrices of
tests/information_reference.py.  Every function takes `dtype` (np.float64, or np.longdouble as a yardstick).

Data.  n node poses T_i (4 x 4, node i's frame -> the common frame); m edges (s, t, X, L, uncertain): X aligns s to t,
so a consistent graph has T_t^-1 T_s = X; L is the 6 x 6 information matrix (upper triangle read, taken symmetric),
rotation block first.
  V(xi)      xi = (a, b, c, tx, ty, tz): R = Rz(c) Ry(b) Rx(a), translation (tx, ty, tz)  (TransformVector6dToMatrix4d)
  v6(M)      its inverse (TransformMatrix4dToVector6d): sy = sqrt(M00^2 + M10^2); sy > 1e-6: a = atan2(M21, M22),
             b = atan2(-M20, sy), c = atan2(M10, M00); otherwise a = atan2(-M12, M11), b = atan2(-M20, sy), c = 0;
             then the translation
  edge k     e_k = v6(X^-1 T_t^-1 T_s),  r_k = e_k^T L e_k;  l_k = 1 (certain) or (mu / (mu + r_k))^2 (uncertain)
  F          SUM l_k r_k + SUM_uncertain mu (sqrt(l_k) - 1)^2
  mu         preference_loop_closure * max_correspondence_distance^2 * mean over the pass's uncertain edges of
             L(5,5); 0 without uncertain edges; fixed per pass from the graph the pass starts with
  Jacobian   left perturbation T_i <- V(d_i) T_i:  J_s[:, c] = lin6(X^-1 T_t^-1 D_c T_s), D_c the six generators of V
             at 0, lin6(M) = ((M21 - M12)/2, (M02 - M20)/2, (M10 - M01)/2, M03, M13, M23);  J_t = -J_s.  (Open3D's
             linearisation: the derivative of e_k where e_k = 0, an approximation elsewhere.)
  system     H accumulates l_k J^T L J into blocks (s,s), (t,t), (s,t), (t,s); g accumulates l_k J^T L e_k; diagonal
             blocks in ascending edge index.  The reference node is held: its six unknowns are left out.
LM loop of one pass (tau = 1e-5), in trials; T, F, H, g belong to the current poses:
  start      lam = tau * max diag H, nu = 2, it = 0, lm = 0;  |g|inf <= min_right_term -> stop RIGHT_TERM
  trial      solve (H + lam I) d = -g by Cholesky; a pivot that is not finite or not positive -> rejected step
             |d|2 <= min_relative_increment (|x|2 + min_relative_increment), x the stacked v6 of the free poses
                 -> stop INCREMENT
             T' = V(d_i) T_i, F' = F(T'), rho = (F - F') / d^T (lam d - g)
             rho > 0:  F - F' < min_relative_residual_increment F -> stop REL_RESIDUAL (the step is not taken)
                       accept: lam *= max(lower_scale_factor, min(upper_scale_factor, 1 - (2 rho - 1)^3)), nu = 2,
                       T = T', relinearise; |g|inf <= min_right_term -> stop RIGHT_TERM; it += 1, lm = 0;
                       F < min_residual -> stop RESIDUAL; it >= max_iteration -> stop MAX_ITERATION
             else      (also a failed factorisation) lam *= nu, nu *= 2, lm += 1;
                       lm >= max_iteration_lm -> stop MAX_ITERATION_LM
Two passes: after pass one every uncertain edge with l_k < edge_prune_threshold (l_k at the final poses) is pruned; if
any was, pass two runs from pass one's poses without them.  edge_prune_threshold = 0: one pass.  n = 1 or m = 0
returns the input (status TRIVIAL)."""
import numpy as np

RIGHT_TERM, INCREMENT, REL_RESIDUAL, RESIDUAL, MAX_ITERATION, MAX_ITERATION_LM, TRIVIAL = range(7)
TAU = 1e-5

DEFAULTS = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6,
                min_relative_residual_increment=1e-6, min_right_term=1e-6, min_residual=1e-6,
                upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0, max_correspondence_distance=0.03,
                edge_prune_threshold=0.25, preference_loop_closure=1.0, reference_node=-1)


def V(xi, dtype=np.float64):
    xi = np.asarray(xi, dtype=dtype)
    ca, sa, cb, sb, cg, sg = np.cos(xi[0]), np.sin(xi[0]), np.cos(xi[1]), np.sin(xi[1]), np.cos(xi[2]), np.sin(xi[2])
    M = np.zeros((4, 4), dtype=dtype)
    M[0, :3] = [cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa]
    M[1, :3] = [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa]
    M[2, :3] = [-sb, cb * sa, cb * ca]
    M[:3, 3] = xi[3:]
    M[3, 3] = 1
    return M


def v6(M, dtype=np.float64):
    M = np.asarray(M, dtype=dtype)
    sy = np.sqrt(M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0])
    out = np.zeros(6, dtype=dtype)
    if sy > 1e-6:
        out[0] = np.arctan2(M[2, 1], M[2, 2])
        out[1] = np.arctan2(-M[2, 0], sy)
        out[2] = np.arctan2(M[1, 0], M[0, 0])
    else:
        out[0] = np.arctan2(-M[1, 2], M[1, 1])
        out[1] = np.arctan2(-M[2, 0], sy)
        out[2] = 0
    out[3:] = M[:3, 3]
    return out


def inverse(T):
    out = np.zeros_like(T)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    out[3, 3] = 1
    return out


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3],
                     M[2, 3]], dtype=M.dtype)


def generators(dtype=np.float64):
    D = np.zeros((6, 4, 4), dtype=dtype)
    D[0, 1, 2], D[0, 2, 1] = -1, 1
    D[1, 0, 2], D[1, 2, 0] = 1, -1
    D[2, 0, 1], D[2, 1, 0] = -1, 1
    D[3, 0, 3] = D[4, 1, 3] = D[5, 2, 3] = 1
    return D


def symmetric(L, dtype):
    U = np.triu(np.asarray(L, dtype=dtype))
    return U + np.triu(U, 1).T


def line_weight(mu, r, uncertain):
    if not uncertain:
        return r.dtype.type(1)
    q = mu / (mu + r)
    return q * q


def line_process_weight(edges, opt, dtype=np.float64):
    counts = [np.asarray(E[3], dtype=dtype)[5, 5] for E in edges if E[4]]
    if not counts:
        return dtype(0)
    mcd = dtype(opt["max_correspondence_distance"])
    return dtype(opt["preference_loop_closure"]) * mcd * mcd * (sum(counts) / dtype(len(counts)))


def residuals(poses, edges, mu, dtype=np.float64):
    """e (m x 6), r (m), l (m), F."""
    m = len(edges)
    e = np.zeros((m, 6), dtype=dtype)
    r = np.zeros(m, dtype=dtype)
    l = np.ones(m, dtype=dtype)
    F = dtype(0)
    for k, (s, t, X, L, unc) in enumerate(edges):
        E = inverse(np.asarray(X, dtype=dtype)) @ inverse(poses[t]) @ poses[s]
        e[k] = v6(E, dtype)
        r[k] = e[k] @ symmetric(L, dtype) @ e[k]
        l[k] = line_weight(mu, r[k], unc)
        F = F + l[k] * r[k]
        if unc:
            F = F + mu * (np.sqrt(l[k]) - 1) ** 2
    return e, r, l, F


def jacobian(poses, edge, dtype=np.float64):
    s, t, X = edge[0], edge[1], np.asarray(edge[2], dtype=dtype)
    A = inverse(X) @ inverse(poses[t])
    return np.stack([lin6(A @ D @ poses[s]) for D in generators(dtype)], axis=1)  # J_s; J_t = -J_s


def linearize(poses, edges, opt=None, dtype=np.float64, mu=None):
    """dict(e, r, l, mu, F, H (6n x 6n, reference rows and columns zero), g (6n))."""
    opt = dict(DEFAULTS, **(opt or {}))
    poses = np.asarray(poses, dtype=dtype)
    n = len(poses)
    ref = 0 if opt["reference_node"] < 0 else opt["reference_node"]
    mu = line_process_weight(edges, opt, dtype) if mu is None else mu
    e, r, l, F = residuals(poses, edges, mu, dtype)
    H = np.zeros((6 * n, 6 * n), dtype=dtype)
    g = np.zeros(6 * n, dtype=dtype)
    for k, E in enumerate(edges):
        s, t = E[0], E[1]
        J = jacobian(poses, E, dtype)
        L = symmetric(E[3], dtype)
        A = l[k] * (J.T @ L @ J)
        b = l[k] * (J.T @ (L @ e[k]))
        S, T = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        H[S, S] += A
        H[T, T] += A
        H[S, T] -= A
        H[T, S] -= A.T
        g[S] += b
        g[T] -= b
    R = slice(6 * ref, 6 * ref + 6)
    H[R, :] = 0
    H[:, R] = 0
    g[R] = 0
    return dict(e=e, r=r, l=l, mu=mu, F=F, H=H, g=g)


def cholesky_solve(A, b):
    """x with A x = b by Cholesky, or None when a pivot is not finite or not positive.  Plain loops over columns, so
    that it runs in any dtype."""
    n = len(b)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not np.isfinite(d) or not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def free_indices(n, ref):
    return np.concatenate([np.arange(6 * i, 6 * i + 6) for i in range(n) if i != ref]).astype(np.int64)


def first_step(poses, edges, opt=None, dtype=np.float64):
    """The first trial's lam and d (6n, zero at the reference node) of a pass; d None when the factorisation fails."""
    opt = dict(DEFAULTS, **(opt or {}))
    lin = linearize(poses, edges, opt, dtype)
    n = len(poses)
    ref = 0 if opt["reference_node"] < 0 else opt["reference_node"]
    idx = free_indices(n, ref)
    lam = dtype(TAU) * np.max(np.diag(lin["H"])[idx])
    A = lin["H"][np.ix_(idx, idx)] + lam * np.eye(len(idx), dtype=dtype)
    x = cholesky_solve(A, -lin["g"][idx])
    d = None
    if x is not None:
        d = np.zeros(6 * n, dtype=dtype)
        d[idx] = x
    return dict(lin, lam=lam, d=d, A=A)


def optimize_pass(poses, edges, opt, dtype=np.float64):
    """One pass.  dict(poses, F0, F, iterations, status, trace, l, mu); trace: one dict per trial and per stop test
    evaluated, for the margin checks of the tests."""
    poses = np.array(poses, dtype=dtype)
    n = len(poses)
    ref = 0 if opt["reference_node"] < 0 else opt["reference_node"]
    idx = free_indices(n, ref)
    mu = line_process_weight(edges, opt, dtype)
    lin = linearize(poses, edges, opt, dtype, mu)
    F0 = F = lin["F"]
    trace = []

    def test(name, value, threshold, fires):
        trace.append(dict(kind="test", name=name, value=float(value), threshold=float(threshold), fires=bool(fires)))
        return fires

    def done(status, it):
        e, r, l, _ = residuals(poses, edges, mu, dtype)
        return dict(poses=poses, F0=F0, F=F, iterations=it, status=status, trace=trace, l=l, mu=mu)

    H, g = lin["H"][np.ix_(idx, idx)], lin["g"][idx]
    lam = dtype(TAU) * np.max(np.diag(H))
    nu = dtype(2)
    it = lm = 0
    gmax = np.max(np.abs(g))
    if test("right_term", gmax, opt["min_right_term"], gmax <= opt["min_right_term"]):
        return done(RIGHT_TERM, it)
    while True:
        x = cholesky_solve(H + lam * np.eye(len(idx), dtype=dtype), -g)
        rho = None
        if x is not None:
            xnorm = np.sqrt(sum(v6(poses[i], dtype) @ v6(poses[i], dtype) for i in range(n) if i != ref))
            dnorm = np.sqrt(x @ x)
            bound = dtype(opt["min_relative_increment"]) * (xnorm + dtype(opt["min_relative_increment"]))
            if test("increment", dnorm, bound, dnorm <= bound):
                return done(INCREMENT, it)
            d = np.zeros(6 * n, dtype=dtype)
            d[idx] = x
            cand = np.stack([V(d[6 * i:6 * i + 6], dtype) @ poses[i] for i in range(n)])
            Fn = residuals(cand, edges, mu, dtype)[3]
            rho = (F - Fn) / (x @ (lam * x - g))
        trace.append(dict(kind="trial", rho=None if rho is None else float(rho), accepted=bool(rho is not None and rho > 0),
                          lam=float(lam)))
        if rho is not None and rho > 0:
            rel = dtype(opt["min_relative_residual_increment"]) * F
            if test("rel_residual", F - Fn, rel, F - Fn < rel):
                return done(REL_RESIDUAL, it)
            alpha = 1 - (2 * rho - 1) ** 3
            lam = lam * max(dtype(opt["lower_scale_factor"]), min(dtype(opt["upper_scale_factor"]), alpha))
            nu = dtype(2)
            poses, F = cand, Fn
            lin = linearize(poses, edges, opt, dtype, mu)
            H, g = lin["H"][np.ix_(idx, idx)], lin["g"][idx]
            gmax = np.max(np.abs(g))
            if test("right_term", gmax, opt["min_right_term"], gmax <= opt["min_right_term"]):
                return done(RIGHT_TERM, it)
            it, lm = it + 1, 0
            if test("residual", F, opt["min_residual"], F < opt["min_residual"]):
                return done(RESIDUAL, it)
            if it >= opt["max_iteration"]:
                return done(MAX_ITERATION, it)
        else:
            lam, nu, lm = lam * nu, nu * 2, lm + 1
            if lm >= opt["max_iteration_lm"]:
                return done(MAX_ITERATION_LM, it)


def global_optimization(poses, edges, opt=None, dtype=np.float64):
    """dict(poses, confidence (m, final l_k; of a pruned edge its value when it was pruned), pruned (m bool), F0, F,
    iterations (per pass), status, passes (the optimize_pass results))."""
    opt = dict(DEFAULTS, **(opt or {}))
    poses = np.array(poses, dtype=dtype)
    m = len(edges)
    pruned = np.zeros(m, dtype=bool)
    if len(poses) <= 1 or m == 0:
        return dict(poses=poses, confidence=np.ones(m, dtype=dtype), pruned=pruned, F0=dtype(0), F=dtype(0),
                    iterations=[0, 0], status=TRIVIAL, passes=[])
    one = optimize_pass(poses, edges, opt, dtype)
    conf = one["l"].copy()
    passes = [one]
    if opt["edge_prune_threshold"] > 0:
        pruned = np.array([bool(E[4]) and conf[k] < opt["edge_prune_threshold"] for k, E in enumerate(edges)])
    if pruned.any():
        keep = np.flatnonzero(~pruned)
        two = optimize_pass(one["poses"], [edges[k] for k in keep], opt, dtype)
        conf[keep] = two["l"]
        passes.append(two)
    last = passes[-1]
    return dict(poses=last["poses"], confidence=conf, pruned=pruned, F0=one["F0"], F=last["F"],
                iterations=[one["iterations"], passes[1]["iterations"] if len(passes) > 1 else 0], status=last["status"],
                passes=passes)


def chain_odometry(poses, edges, ref=0):
    """Poses obtained by chaining the certain edges (i -> i + 1) alone from the reference node's input pose."""
    out = np.array(poses)
    by_pair = {(E[0], E[1]): np.asarray(E[2]) for E in edges if not E[4]}
    for i in range(ref + 1, len(out)):  # T_{i-1}^-1 T_i = X(i -> i-1) or its inverse
        if (i, i - 1) in by_pair:
            out[i] = out[i - 1] @ by_pair[(i, i - 1)]
        else:
            out[i] = out[i - 1] @ inverse(by_pair[(i - 1, i)])
    for i in range(ref - 1, -1, -1):
        if (i, i + 1) in by_pair:
            out[i] = out[i + 1] @ by_pair[(i, i + 1)]
        else:
            out[i] = out[i + 1] @ inverse(by_pair[(i + 1, i)])
    return out
