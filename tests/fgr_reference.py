"""Fast Global Registration on correspondences, restated in numpy from the contract in include/teaser_hip.h ("Fast
Global Registration on correspondences"): every expression with the contract's parentheses, every sum in the contract's
block order.  dtype selects np.float64 (the device's arithmetic, up to sin / cos / sqrt of the host's libm) or
np.longdouble (the reference the GPU tests compare against).  Open3D is not run; this file IS the comparison."""
import numpy as np

BLOCK = 256
MIN_CORR = 10
_LANE = np.arange(64)


def block_sum(items, dtype=np.float64):
    """The contract's block order over the rows of items (n x m): returns the m sums."""
    x = np.asarray(items, dtype=dtype)
    if x.ndim == 1:
        x = x[:, None]
    return _level(_level(x, dtype), dtype, partials=True)[0]


def _block(v):
    """256 x m -> m: lanes by xor shuffles, then (w0 + w1) + (w2 + w3)."""
    w = v.reshape(4, 64, -1).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, _LANE ^ o, :]
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


def _level(x, dtype, partials=False):
    n, m = x.shape
    if partials:  # accumulator t = 0.0 + x[t] + x[t + 256] + ...
        acc = np.zeros((BLOCK, m), dtype=dtype)
        for first in range(0, n, BLOCK):
            part = x[first:first + BLOCK]
            acc[:len(part)] = acc[:len(part)] + part
        return _block(acc)[None, :]
    nblk = (n + BLOCK - 1) // BLOCK
    pad = np.zeros((nblk * BLOCK, m), dtype=dtype)
    pad[:n] = x
    return np.stack([_block(pad[b * BLOCK:(b + 1) * BLOCK]) for b in range(nblk)]) if nblk else np.zeros((0, m), dtype)


def rotation(xi, dtype=np.float64):
    """delta = [Rz(xi2) Ry(xi1) Rx(xi0) | xi3..5] as a 4 x 4, the entries written as the ICP contract's."""
    xi = np.asarray(xi, dtype=dtype)
    ca, sa, cb, sb, cg, sg = np.cos(xi[0]), np.sin(xi[0]), np.cos(xi[1]), np.sin(xi[1]), np.cos(xi[2]), np.sin(xi[2])
    U = np.zeros((4, 4), dtype=dtype)
    U[0, :3] = [cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa]
    U[1, :3] = [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa]
    U[2, :3] = [-sb, cb * sa, cb * ca]
    U[:3, 3] = xi[3:6]
    U[3, 3] = 1
    return U


def apply(U, x):
    """apply(U, x) of the ICP contract on the rows of x."""
    return np.stack([((U[r, 0] * x[:, 0] + U[r, 1] * x[:, 1]) + U[r, 2] * x[:, 2]) + U[r, 3] for r in range(3)], axis=1)


def compose(U, T):
    """delta trans with the contract's parentheses."""
    out = T.copy()
    for r in range(3):
        out[r] = ((U[r, 0] * T[0] + U[r, 1] * T[1]) + U[r, 2] * T[2]) + U[r, 3] * T[3]
    return out


def jacobian_rows(q):
    """The three rows J0, J1, J2 of one record q."""
    z = 0 * q[0]
    return np.array([[z, -q[2], q[1], -1 + z, z, z], [q[2], z, -q[0], z, -1 + z, z], [-q[1], q[0], z, z, z, -1 + z]])


def terms(p, q, mu, dtype=np.float64):
    """The 27 terms of every pair (n x 27): A's upper triangle by rows, then g."""
    p, q = np.asarray(p, dtype=dtype), np.asarray(q, dtype=dtype)
    mu = dtype(mu)
    e0, e1, e2 = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
    t = mu / (((e0 * e0 + e1 * e1) + e2 * e2) + mu)
    s = t * t
    q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
    zero = np.zeros_like(s)
    v = [s * (q2 * q2 + q1 * q1), s * (0 - q1 * q0), s * (0 - q2 * q0), zero, s * (0 - q2), s * q1,
         s * (q2 * q2 + q0 * q0), s * (0 - q2 * q1), s * q2, zero, s * (0 - q0),
         s * (q1 * q1 + q0 * q0), s * (0 - q1), s * q0, zero,
         s, zero, zero, s, zero, s,
         s * (e1 * q2 - e2 * q1), s * (e2 * q0 - e0 * q2), s * (e0 * q1 - e1 * q0),
         s * (0 - e0), s * (0 - e1), s * (0 - e2)]
    return np.stack(v, axis=1)


def unpack(tot):
    """The 27 sums -> (A 6 x 6 mirrored, g 6)."""
    A = np.zeros((6, 6), dtype=tot.dtype)
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = tot[k]
            k += 1
    return A, tot[21:27].copy()


def solve(A, g):
    """A xi = -g by LDL^T without pivoting, the recurrences of point-to-plane ICP.  Returns (xi, failed)."""
    dtype = A.dtype.type
    L = np.zeros((6, 6), dtype=dtype)
    dd = np.zeros(6, dtype=dtype)
    xi = np.zeros(6, dtype=dtype)
    for j in range(6):
        sj = A[j, j]
        for m in range(j):
            sj = sj - L[j, m] * L[j, m] * dd[m]
        if not np.isfinite(sj) or not sj > 0:
            return xi, 1
        dd[j] = sj
        for i in range(j + 1, 6):
            t = A[i, j]
            for m in range(j):
                t = t - L[i, m] * L[j, m] * dd[m]
            L[i, j] = t / sj
    y = np.zeros(6, dtype=dtype)
    for i in range(6):
        t = -g[i]
        for m in range(i):
            t = t - L[i, m] * y[m]
        y[i] = t
    y = y / dd
    for i in range(5, -1, -1):
        t = y[i]
        for m in range(i + 1, 6):
            t = t - L[m, i] * xi[m]
        xi[i] = t
    return xi, 0 if np.all(np.isfinite(xi)) else 1


def normalise(P, Q, corr, use_absolute_scale=False, dtype=np.float64):
    """dict: mean_p, mean_q, scale, scale_global, scale_start, p (ncorr x 3), q (ncorr x 3), zero_scale."""
    P, Q = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    corr = np.asarray(corr, dtype=np.int64).reshape(-1, 2)
    mp, mq = block_sum(P, dtype) / dtype(len(P)), block_sum(Q, dtype) / dtype(len(Q))
    scale = dtype(0)
    for X, m in ((P, mp), (Q, mq)):
        d = X - m
        scale = max(scale, np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
    sg, ss = (dtype(1), scale) if use_absolute_scale else (scale, dtype(1))
    zero = not scale > 0
    if zero:
        p, q = np.zeros((len(corr), 3), dtype=dtype), np.zeros((len(corr), 3), dtype=dtype)
    else:
        p, q = (P[corr[:, 0]] - mp) / sg, (Q[corr[:, 1]] - mq) / sg
    return dict(mean_p=mp, mean_q=mq, scale=scale, scale_global=sg, scale_start=ss, p=p, q=q, zero_scale=zero)


def mu_schedule(mu, iteration_number, division_factor=1.4, maximum_correspondence_distance=0.025, decrease_mu=True):
    """The mu each iteration uses, then the final one: scalar IEEE divisions (Python floats)."""
    used, mu = [], float(mu)
    for itr in range(iteration_number):
        used.append(mu)
        if decrease_mu and itr % 4 == 0 and mu > maximum_correspondence_distance:
            mu = mu / division_factor
    return used, mu


def finish(trans, mean_p, mean_q, scale_global):
    """T (source -> target in the caller's frame) from trans: the rigid inverse of M."""
    dtype = trans.dtype.type
    R, t = trans[:3, :3], trans[:3, 3]
    tm = np.array([(t[r] * scale_global - ((R[r, 0] * mean_q[0] + R[r, 1] * mean_q[1]) + R[r, 2] * mean_q[2])) + mean_p[r]
                   for r in range(3)], dtype=dtype)
    T = np.zeros((4, 4), dtype=dtype)
    T[:3, :3] = R.T
    for r in range(3):
        T[r, 3] = 0 - ((R[0, r] * tm[0] + R[1, r] * tm[1]) + R[2, r] * tm[2])
    T[3, 3] = 1
    return T


def fgr(P, Q, corr, division_factor=1.4, use_absolute_scale=False, decrease_mu=True,
        maximum_correspondence_distance=0.025, iteration_number=64, dtype=np.float64, n=None):
    """The whole contract (n: stop after the first n iterations, as the stage call does).  dict: transformation,
    optimised, scale_global, scale_start, final_mu, iterations, failed_solves, flags, mean_p, mean_q, scale, p, q (the
    moved records) and per iteration mu, A, g, xi, flag, trans."""
    nm = normalise(P, Q, corr, use_absolute_scale, dtype)
    p, q = nm["p"], nm["q"].copy()
    ncorr = len(p)
    trans = np.eye(4, dtype=dtype)
    mu = dtype(nm["scale_start"])
    flags = (1 if ncorr < MIN_CORR else 0) | (2 if nm["zero_scale"] else 0)
    log = dict(mu=[], A=[], g=[], xi=[], flag=[], trans=[])
    failed = 0
    steps = 0 if flags else (iteration_number if n is None else n)
    div, maxd = dtype(division_factor), dtype(maximum_correspondence_distance)
    for itr in range(steps):
        A, g = unpack(block_sum(terms(p, q, mu, dtype), dtype))
        xi, bad = solve(A, g)
        U = np.eye(4, dtype=dtype) if bad else rotation(xi, dtype)
        failed += bad
        trans = compose(U, trans)
        q = apply(U, q)
        log["mu"].append(mu)
        log["A"].append(A)
        log["g"].append(g)
        log["xi"].append(xi)
        log["flag"].append(bad)
        log["trans"].append(trans.copy())
        if decrease_mu and itr % 4 == 0 and mu > maxd:
            mu = mu / div
    T = finish(trans, nm["mean_p"], nm["mean_q"], nm["scale_global"])
    out = dict(transformation=T, optimised=trans, scale_global=nm["scale_global"], scale_start=nm["scale_start"],
               final_mu=mu, iterations=steps, failed_solves=failed, flags=flags, mean_p=nm["mean_p"],
               mean_q=nm["mean_q"], scale=nm["scale"], p=p, q=q)
    out.update({k: (np.array(v) if v else np.zeros((0,), dtype=dtype)) for k, v in log.items()})
    return out


# ---- the shapes the fixture and the GPU tests share ----
def rot_z_y(a, b):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1.0]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])


def make_case(seed, n_s, n_t, ncorr, outlier=0.3, noise=1e-3, repeats=True):
    """A problem with a known pose: Q[j] = R P[i] + t (+ noise) on the inlier pairs, uniform outliers elsewhere.
    Returns P, Q, corr (int32), T_true (4 x 4, source -> target)."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1, 1, (n_s, 3)) + np.array([0.3, -0.2, 0.5])
    R, t = rot_z_y(0.4 + 0.1 * (seed % 5), -0.3), np.array([0.25, -0.4, 0.15])
    Q = rng.uniform(-1.5, 1.5, (n_t, 3))
    m = min(n_s, n_t, ncorr)
    i = rng.permutation(n_s)[:m]
    j = rng.permutation(n_t)[:m]
    n_in = m - int(round(outlier * m))
    Q[j[:n_in]] = P[i[:n_in]] @ R.T + t + noise * rng.standard_normal((n_in, 3))
    corr = np.stack([i, j], axis=1)
    if ncorr > m:  # more pairs than points: repeats of the pairs above
        corr = np.concatenate([corr, corr[rng.integers(0, m, ncorr - m)]])
    elif repeats and ncorr >= 4:
        corr[-1] = corr[0]
    corr = corr[rng.permutation(len(corr))]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return P, Q, np.ascontiguousarray(corr, dtype=np.int32), T


# name: (seed, n_s, n_t, ncorr, options)
CASES = {
    "c9": (1, 40, 57, 9, {}),
    "c10": (2, 40, 300, 10, {}),
    "c63": (3, 255, 64, 63, {}),
    "c64": (4, 256, 257, 64, {"iteration_number": 5}),
    "c65": (5, 257, 1025, 65, {"decrease_mu": False}),
    "c255": (6, 1024, 300, 255, {"use_absolute_scale": True}),
    "c256": (7, 1500, 1023, 256, {"maximum_correspondence_distance": 0.3}),
    "c257": (8, 300, 1500, 257, {"iteration_number": 1}),
    "c1025": (9, 700, 900, 1025, {}),
    "c257_it0": (10, 300, 280, 257, {"iteration_number": 0}),
}


def case(name):
    seed, n_s, n_t, ncorr, opt = CASES[name]
    P, Q, corr, T = make_case(seed, n_s, n_t, ncorr)
    return P, Q, corr, T, dict(opt)


# ---- the batch tests/test_gpu_wide_batches.py and tests/test_wide_batch_cases.py share ----
WIDE_BATCH = 320
WIDE_STAGE = 3  # iterations of the wide test's stage call
WIDE_SPLIT = 40  # resident_max_corr that sends about half of the batch down each route


def wide_batch():
    """320 problems of 20 .. 60 pairs whose iteration_number cycles over 0 .. 16, so that the list of open problems
    empties unevenly; problem 150 has 5 pairs (fewer than FGR optimises).  Returns (problems, options): (P, Q, corr)
    and the keyword arguments of fgr() per problem.  What the wide test rests on is asserted from the sizes alone."""
    b = WIDE_BATCH
    its = (0, 1, 2, 3, 5, 8, 13, 16, 4)
    problems, options = [], []
    for i in range(b):
        ncorr = 5 if i == 150 else (20, 33, 47, 60)[i % 4]
        P, Q, corr, _ = make_case(4000 + i, ncorr + 7, ncorr + 12, ncorr)
        problems.append((P, Q, corr))
        options.append(dict(iteration_number=its[i % len(its)], use_absolute_scale=bool(i % 5 == 0),
                            decrease_mu=bool(i % 7 != 0), maximum_correspondence_distance=(0.025, 0.3)[i % 2]))
    n = [len(p[2]) for p in problems]
    assert b > 256  # fgr_finish_kernel's second block of 256 threads, blockIdx.y past 255 in fgr_cloud_*
    assert sum(k < MIN_CORR for k in n) == 1 and n[150] < MIN_CORR
    res = [k for k in n if MIN_CORR <= k <= WIDE_SPLIT]
    assert len(res) > 128 and len(n) - len(res) > 128  # both routes' index lists at resident_max_corr = WIDE_SPLIT
    for lo in (0, 256):  # the open list thins out below and above problem 256
        assert len({o["iteration_number"] for o in options[lo:lo + 64]}) == len(its)
    return problems, options
