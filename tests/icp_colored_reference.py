"""numpy restatement of the Colored-ICP contract (include/teaser_hip.h, "ICP refinement: Colored ICP"; DESIGN.md
section 22).  apply, compose and corr -- the loop, the search, fitness, the Euclidean inlier RMSE and the stop rule --
are those of the point-to-point restatement (tests/icp_reference.py); the kernels, the 6 x 6 solve and the step matrix
those of the point-to-plane restatement (tests/icp_plane_reference.py); the neighbourhood of a colour gradient is the
covariance contract's (tests/icp_gicp_reference.py).  What is restated here:

  I = ((r + g) + b) / 3
  gradient of target point i (x, n): slots 1 .. m - 1 of the neighbourhood in list order, o = y - x,
  s = (o0 n0 + o1 n1) + o2 n2, a = o - s n, b = I[j] - I[i], G += a a^T, h += a b one neighbour at a time, then
  G += (w n)(w n)^T with w = m - 1, G d = h by LDL^T without pivoting; 0 when m < 4, a pivot fails or d is not finite.

  step: sg = sqrt(lambda), sp = sqrt(1 - lambda); per correspondence Jg = sg [x' x n ; n], rg = sg s,
  u = e - s n, isp = ((d0 u0 + d1 u1) + d2 u2) + It, t = d . n, dm = t n - d, Ji = sp [x' x dm ; dm],
  ri = sp (Is - isp); A += (wg Jg[r]) Jg[c] + (wi Ji[r]) Ji[c], g += (wg rg) Jg[r] + (wi ri) Ji[r]."""
import numpy as np
from scipy.spatial import cKDTree

from icp_gicp_reference import neighbourhood
from icp_plane_reference import centre_of, margins_of, solve6, step_matrix, weight
from icp_reference import apply, compose, corr


def intensity(colors):
    c = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0


def solve3(G, h):
    """d with G d = h by LDL^T without pivoting (the recurrences of solve6), or zeros."""
    L = np.eye(3)
    d = np.zeros(3)
    for j in range(3):
        s = G[j, j]
        for k in range(j):
            s -= L[j, k] * L[j, k] * d[k]
        if not np.isfinite(s) or not s > 0:
            return np.zeros(3)
        d[j] = s
        for i in range(j + 1, 3):
            t = G[i, j]
            for k in range(j):
                t -= L[i, k] * L[j, k] * d[k]
            L[i, j] = t / s
    y = np.zeros(3)
    for i in range(3):
        t = h[i]
        for k in range(i):
            t -= L[i, k] * y[k]
        y[i] = t
    y = y / d
    x = np.zeros(3)
    for i in range(2, -1, -1):
        t = y[i]
        for k in range(i + 1, 3):
            t -= L[k, i] * x[k]
        x[i] = t
    return x if np.isfinite(x).all() else np.zeros(3)


def color_gradients(points, normals, colors, radius, max_nn=30, details=False):
    """n x 3 gradients, scalar arithmetic, sequential sums in list order.  details=True adds (m per point, the relative
    gap between the max_nn-th and the next d2 per point (inf when max_nn does not bind), the relative distance of the
    nearest d2 to radius^2 per point)."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    N = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    I = intensity(colors)
    n = len(P)
    out = np.zeros((n, 3))
    ms, nn_gap, edge = np.zeros(n, dtype=np.int64), np.full(n, np.inf), np.full(n, np.inf)
    if n == 0:
        return (out, ms, nn_gap, edge) if details else out
    tree = cKDTree(P)
    r2 = radius * radius
    for i in range(n):
        js, d2, nxt = neighbourhood(P, i, radius, max_nn, tree)
        m = len(js)
        ms[i] = m
        if details:
            near = np.asarray(tree.query_ball_point(P[i], radius * 1.01), dtype=np.int64)
            ex, ey, ez = P[i, 0] - P[near, 0], P[i, 1] - P[near, 1], P[i, 2] - P[near, 2]
            edge[i] = np.abs(((ex * ex + ey * ey) + ez * ez) - r2).min() / r2
            if nxt is not None:
                nn_gap[i] = (nxt - d2[-1]) / nxt if nxt > 0 else 0.0
        if m < 4:
            continue
        x, nv = P[i], N[i]
        G = np.zeros((3, 3))
        h = np.zeros(3)
        for j in js[1:]:
            o = P[j] - x
            s = (o[0] * nv[0] + o[1] * nv[1]) + o[2] * nv[2]
            a = o - s * nv
            b = I[j] - I[i]
            for r in range(3):
                for c in range(r, 3):
                    G[r, c] += a[r] * a[c]
                h[r] += a[r] * b
        w = float(m - 1)
        wn = w * nv
        for r in range(3):
            for c in range(r, 3):
                G[r, c] += wn[r] * wn[c]
                G[c, r] = G[r, c]
        out[i] = solve3(G, h)
    return (out, ms, nn_gap, edge) if details else out


def terms(X, Q, N, D, Is, It, c, lam, kernel="l2", k=1.0):
    """What each matched row adds: (m x 6 x 6 symmetric, m x 6)."""
    sg, sp = np.sqrt(lam), np.sqrt(1.0 - lam)
    xp, qp = X - c, Q - c
    e = xp - qp
    s = (e[:, 0] * N[:, 0] + e[:, 1] * N[:, 1]) + e[:, 2] * N[:, 2]

    def jac(v, f):
        J = np.empty((len(X), 6))
        J[:, 0] = f * (xp[:, 1] * v[:, 2] - xp[:, 2] * v[:, 1])
        J[:, 1] = f * (xp[:, 2] * v[:, 0] - xp[:, 0] * v[:, 2])
        J[:, 2] = f * (xp[:, 0] * v[:, 1] - xp[:, 1] * v[:, 0])
        J[:, 3:] = f * v
        return J

    Jg = jac(N, sg)
    rg = sg * s
    wg = weight(kernel, k, rg)
    u = e - s[:, None] * N
    isp = ((D[:, 0] * u[:, 0] + D[:, 1] * u[:, 1]) + D[:, 2] * u[:, 2]) + It
    t = (D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1]) + D[:, 2] * N[:, 2]
    dm = t[:, None] * N - D
    Ji = jac(dm, sp)
    ri = sp * (Is - isp)
    wi = weight(kernel, k, ri)
    tA = (wg[:, None] * Jg)[:, :, None] * Jg[:, None, :] + (wi[:, None] * Ji)[:, :, None] * Ji[:, None, :]
    tg = (wg * rg)[:, None] * Jg + (wi * ri)[:, None] * Ji
    return tA, tg


def _seq(t):
    return np.cumsum(t, axis=0)[-1] if len(t) else np.zeros(t.shape[1:])


def colored_step(X, Q, N, D, Is, It, c, lam, kernel="l2", k=1.0, order=None, chunk=None):
    if len(X) == 0:
        return np.eye(4)
    tA, tg = terms(X, Q, N, D, Is, It, c, lam, kernel, k)
    if order is not None:
        tA, tg = tA[order], tg[order]
    if chunk:
        pa = [_seq(tA[s:s + chunk]) for s in range(0, len(tA), chunk)]
        pg = [_seq(tg[s:s + chunk]) for s in range(0, len(tg), chunk)]
        A, g = _seq(np.array(pa).reshape(-1, 6, 6)), _seq(np.array(pg).reshape(-1, 6))
    else:
        A, g = _seq(tA), _seq(tg)
    xi = solve6(A, g)
    return np.eye(4) if xi is None else step_matrix(xi, c)


def registration_icp(source, target, source_colors, target_colors, target_normals, r, init=None, lam=0.968,
                     kernel="l2", k=1.0, gradient_radius=None, gradient_max_nn=30, gradients=None, max_iteration=30,
                     relative_fitness=1e-6, relative_rmse=1e-6, margins=False, order_seed=None, chunk=None):
    """Returns dict(transformation, fitness, inlier_rmse, correspondence_set, iterations, gradients) (+ 'margins' as
    icp_plane_reference.registration_icp does).  order_seed / chunk: sum A and g in a shuffled order / in chunks."""
    P = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    N = np.asarray(target_normals, dtype=np.float64).reshape(-1, 3)
    Is, It = intensity(source_colors), intensity(target_colors)
    assert N.shape == Q.shape and len(Is) == len(P) and len(It) == len(Q)
    if gradients is None:
        R = 2.0 * r if gradient_radius is None or gradient_radius <= 0 else gradient_radius
        gradients = color_gradients(Q, N, target_colors, R, gradient_max_nn)
    D = np.asarray(gradients, dtype=np.float64).reshape(-1, 3)
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
        jm = j[m]
        U = colored_step(X[m], Q[jm], N[jm], D[jm], Is[m], It[jm], c, lam, kernel, k, order, chunk)
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
    out = dict(transformation=T, fitness=fit, inlier_rmse=rmse, correspondence_set=cs, iterations=it, gradients=D)
    if margins:
        out["margins"] = mg
    return out


# ---- the scene -------------------------------------------------------------------------------------------------------
SCENE_R = 0.08


def _surface(x, y):
    z = 0.05 * np.sin(1.5 * x) * np.cos(1.2 * y)
    zx = 0.05 * 1.5 * np.cos(1.5 * x) * np.cos(1.2 * y)
    zy = -0.05 * 1.2 * np.sin(1.5 * x) * np.sin(1.2 * y)
    n = np.stack([-zx, -zy, np.ones_like(x)], 1)
    return z, n / np.sqrt((n * n).sum(1))[:, None]


def _texture(x, y):
    i = 0.5 + 0.2 * np.sin(4 * x) + 0.2 * np.cos(3 * y)
    return np.stack([i, i, i], 1)


def scene(seed=0, n_src=1500, grid=48):
    """A gently curved, textured surface z = 0.05 sin(1.5 x) cos(1.2 y) over [-1, 1]^2: the target a grid x grid lattice
    with 5e-4 noise (its analytic normals), intensity 0.5 + 0.2 sin 4x + 0.2 cos 3y, the source n_src random surface
    samples moved by the inverse of the true pose (1 degree about z plus (0.03, -0.02, 0.002)).  Geometry alone lets
    the pose slide along the surface; the texture pins it.  Returns dict(source, target, source_colors, target_colors,
    target_normals, T_true, r)."""
    rng = np.random.default_rng(1000 + seed)
    gx, gy = np.meshgrid(np.linspace(-1, 1, grid), np.linspace(-1, 1, grid))
    gx, gy = gx.ravel(), gy.ravel()
    gz, gn = _surface(gx, gy)
    target = np.stack([gx, gy, gz], 1) + 5e-4 * rng.standard_normal((grid * grid, 3))
    sx, sy = rng.uniform(-0.9, 0.9, n_src), rng.uniform(-0.9, 0.9, n_src)
    sz, _ = _surface(sx, sy)
    world = np.stack([sx, sy, sz], 1)
    a = np.deg2rad(1.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [0.03, -0.02, 0.002]
    source = (world - T[:3, 3]) @ T[:3, :3]  # T maps source onto the surface
    return dict(source=np.ascontiguousarray(source), target=np.ascontiguousarray(target),
                source_colors=_texture(sx, sy), target_colors=_texture(target[:, 0], target[:, 1]),
                target_normals=np.ascontiguousarray(gn), T_true=T, r=SCENE_R)


# ---- the batch tests/test_gpu_wide_batches.py and tests/test_wide_batch_cases.py share ----
WIDE_BATCH = 320
WIDE_R = 0.45  # above the coarsest lattice's spacing (2 / 5), so every gradient has its four neighbours inside 2 r
WIDE_KERNELS = (("huber", 0.002), ("cauchy", 0.002), ("tukey", 0.01))  # the robust kernels, in turn
WIDE_ITERATIONS = 3


def wide_batch():
    """320 textured scenes cut down to 36, 49 or 64 target points and 40 to 120 source points (one without source
    points, one without target points): a list of scene() dicts with r = WIDE_R and the robust kernel of the problem
    as "kernel".  What the wide test rests on is asserted from the sizes alone."""
    b = WIDE_BATCH
    grids = [(6, 7, 8)[i % 3] for i in range(b)]
    n_src = [(40, 97, 120, 60)[i % 4] for i in range(b)]
    assert b > 256 and max(g * g for g in grids) <= 200 and max(n_src) <= 200
    assert len({(grids[i], n_src[i]) for i in (255, 256, 257)}) == 3
    out = []
    for i in range(b):
        s = dict(scene(seed=100 + i, n_src=n_src[i], grid=grids[i]), r=WIDE_R, kernel=WIDE_KERNELS[i % len(WIDE_KERNELS)])
        if i == 130:
            s.update(source=np.zeros((0, 3)), source_colors=np.zeros((0, 3)))
        if i == 190:
            s.update(target=np.zeros((0, 3)), target_colors=np.zeros((0, 3)), target_normals=np.zeros((0, 3)))
        out.append(s)
    # one block of 256 points per non-empty cloud: the gradient kernel's block map holds more than 256 entries
    assert sum((len(s["target"]) + 255) // 256 for s in out) > 256
    return out
