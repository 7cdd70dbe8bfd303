"""The numpy restatement of the depth odometry contract (include/teaser_hip.h, "Depth odometry"), line by line: float32
numpy arrays where the contract says float32, float64 elsewhere, the operations in the order written, the sums in the
tree of blocks and groups of "RGB-D odometry" (ordered_sum, solve, update and the scene come from
tests/odometry_reference.py).  tests/test_depth_odometry_reference.py pins it by facts worked out by hand; the host
driver and the GPU must EQUAL it bit for bit.  Also the one list of cases every depth odometry test shares, with the
results memoised (``result``, ``pyramid``)."""
from types import SimpleNamespace

import numpy as np

import odometry_reference as O
from odometry_reference import QNAN32, canon32, canon64, f32, f64, halved, ordered_sum, solve, update

SUMS = O.SUMS
PLANES = ("D_s", "D_t", "Vs_x", "Vs_y", "Vs_z", "Vt_x", "Vt_y", "Vt_z", "Nt_x", "Nt_y", "Nt_z")
KERNEL = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))


def option(iterations=(10, 5, 3), depth_outlier_trunc=0.07, depth_huber_delta=0.05, depth_min=0.0, depth_max=3.0,
           relative_rmse=1e-6, relative_fitness=1e-6):
    return SimpleNamespace(iterations=tuple(iterations), trunc=depth_outlier_trunc, delta=depth_huber_delta,
                           depth_min=depth_min, depth_max=depth_max, relative_rmse=relative_rmse,
                           relative_fitness=relative_fitness)


# ---- images -----------------------------------------------------------------------------------------------------------
def convert(depth, depth_scale, depth_min, depth_max):
    """Step 1."""
    zf = depth.astype(f32) / f32(depth_scale) if depth.dtype == np.uint16 else np.array(depth, dtype=f32)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(zf) | (zf.astype(f64) <= depth_min) | (zf.astype(f64) > depth_max)
    zf[bad] = QNAN32
    return zf


def pyr_down(D, trunc):
    """Step 2: level l + 1 of one image from level l."""
    h, w = D.shape
    H, W = h // 2, w // 2
    thr = f32(2.0 * trunc)
    c = D[0:2 * H:2, 0:2 * W:2]
    s, ws = np.zeros((H, W), f32), np.zeros((H, W), f32)
    ys, xs = np.meshgrid(2 * np.arange(H), 2 * np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                yy, xx = ys + dy, xs + dx
                inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                v = D[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
                ok = inside & ~np.isnan(v) & (np.abs(v - c) < thr)
                wgt = KERNEL[dy + 2] * KERNEL[dx + 2]
                s = np.where(ok, s + wgt * v, s)
                ws = np.where(ok, ws + wgt, ws)
        out = s / ws
    out = np.where(np.isnan(c), QNAN32, out)
    return canon32(out)


def vertex_map(D, K, l):
    """Step 3: (X, Y, Z) of one image at level l."""
    fx, fy, cx, cy = (halved(v, l) for v in K)
    h, w = D.shape
    xs, ys = np.meshgrid(np.arange(w, dtype=f64), np.arange(h, dtype=f64))
    with np.errstate(all="ignore"):
        X = canon32((((xs - cx) * D.astype(f64)) * (1.0 / fx)).astype(f32))
        Y = canon32((((ys - cy) * D.astype(f64)) * (1.0 / fy)).astype(f32))
    return X, Y, D.copy()


def normal_map(V):
    """Step 4 from the three planes of a vertex map."""
    h, w = V[0].shape
    N = [np.full((h, w), QNAN32, dtype=f32) for _ in range(3)]
    if h < 2 or w < 2:
        return N
    v0 = [p[:-1, :-1] for p in V]
    v1 = [p[:-1, 1:] for p in V]
    v2 = [p[1:, :-1] for p in V]
    ok = np.ones((h - 1, w - 1), bool)
    for p in v0 + v1 + v2:
        ok &= ~np.isnan(p)
    with np.errstate(all="ignore"):
        a = [(v1[c] - v0[c]).astype(f64) for c in range(3)]
        b = [(v2[c] - v0[c]).astype(f64) for c in range(3)]
        m = [b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]]
        ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        ok &= (ln != 0.0) & np.isfinite(ln)
        for c in range(3):
            N[c][:-1, :-1] = np.where(ok, canon32((m[c] / ln).astype(f32)), QNAN32)
    return N


def build_pyramid(pair, opt):
    """Steps 1 .. 4: a list of levels, each a dict plane name -> float32 image."""
    L = len(opt.iterations)
    Ds = [convert(pair.source_depth, pair.depth_scale, opt.depth_min, opt.depth_max)]
    Dt = [convert(pair.target_depth, pair.depth_scale, opt.depth_min, opt.depth_max)]
    for _ in range(L - 1):
        Ds.append(pyr_down(Ds[-1], opt.trunc))
        Dt.append(pyr_down(Dt[-1], opt.trunc))
    levels = []
    for l in range(L):
        Vs, Vt = vertex_map(Ds[l], pair.K, l), vertex_map(Dt[l], pair.K, l)
        Nt = normal_map(Vt)
        levels.append(dict(zip(PLANES, (Ds[l], Dt[l]) + tuple(Vs) + tuple(Vt) + tuple(Nt))))
    return levels


def pyramid_floats(levels):
    """The layout of images_out."""
    return np.concatenate([lev[name].ravel() for lev in levels for name in PLANES])


# ---- one iteration ----------------------------------------------------------------------------------------------------
def project(K, T, l, lev):
    """The projection of step 5: (source pixels s, p (3 arrays), target pixels) of the pixels that are not skipped."""
    fx, fy, cx, cy = (halved(v, l) for v in K)
    h, w = lev["D_s"].shape
    P = [lev[n].ravel() for n in ("Vs_x", "Vs_y", "Vs_z")]
    s = np.flatnonzero(~(np.isnan(P[0]) | np.isnan(P[1]) | np.isnan(P[2])))
    P = [p[s].astype(f64) for p in P]
    T = np.asarray(T, dtype=f64)
    with np.errstate(all="ignore"):
        p = [((T[r, 0] * P[0] + T[r, 1] * P[1]) + T[r, 2] * P[2]) + T[r, 3] for r in range(3)]
        ok = p[2] > 0.0
        x, y = ((fx * p[0]) / p[2] + cx) + 0.5, ((fy * p[1]) / p[2] + cy) + 0.5
        ok &= (x >= 0.0) & (x < 2147483648.0) & (y >= 0.0) & (y < 2147483648.0)
        ut, vt = np.trunc(np.where(ok, x, 0.0)).astype(np.int64), np.trunc(np.where(ok, y, 0.0)).astype(np.int64)
        ok &= (ut < w) & (vt < h)
    return s[ok], [q[ok] for q in p], (vt * w + ut)[ok]


def pixel_values(p, Q, N, trunc, delta):
    """The 29 values of pixels that passed the projection and whose Q and N are free of NaN: (keep mask, values)."""
    with np.errstate(all="ignore"):
        r = ((p[0] - Q[0]) * N[0] + (p[1] - Q[1]) * N[1]) + (p[2] - Q[2]) * N[2]
        keep = np.abs(r) <= trunc
        J = [(-p[2]) * N[1] + p[1] * N[2], p[2] * N[0] - p[0] * N[2], (-p[1]) * N[0] + p[0] * N[1], N[0], N[1], N[2]]
        ar = np.abs(r)
        small = ar < delta
        dh = np.where(small, r, np.where(r < 0.0, -delta, delta))
        lh = np.where(small, (0.5 * r) * r, delta * (ar - 0.5 * delta))
        v = np.zeros((len(r), SUMS))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                v[:, k] = J[i] * J[j]
                k += 1
        for i in range(6):
            v[:, 21 + i] = J[i] * dh
        v[:, 27] = lh
        v[:, 28] = 1.0
    return keep, v


def iteration_sums(K, T, l, lev, opt):
    s, p, tp = project(K, T, l, lev)
    Q = [lev[n].ravel()[tp] for n in ("Vt_x", "Vt_y", "Vt_z")]
    N = [lev[n].ravel()[tp] for n in ("Nt_x", "Nt_y", "Nt_z")]
    ok = np.ones(len(s), bool)
    for a in Q + N:
        ok &= ~np.isnan(a)
    s, p = s[ok], [q[ok] for q in p]
    Q, N = [a[ok].astype(f64) for a in Q], [a[ok].astype(f64) for a in N]
    keep, v = pixel_values(p, Q, N, opt.trunc, opt.delta)
    h, w = lev["D_s"].shape
    return ordered_sum(h * w, s[keep], v[keep])


def information(K, T, lev, opt):
    """Step 6."""
    s, p, tp = project(K, T, 0, lev)
    Q = [lev[n].ravel()[tp] for n in ("Vt_x", "Vt_y", "Vt_z")]
    ok = ~(np.isnan(Q[0]) | np.isnan(Q[1]) | np.isnan(Q[2]))
    s, p, Q = s[ok], [q[ok] for q in p], [a[ok].astype(f64) for a in Q]
    with np.errstate(all="ignore"):
        e = [p[c] - Q[c] for c in range(3)]
        ok = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= opt.trunc * opt.trunc
        s, (x, y, z) = s[ok], [a[ok] for a in Q]
        o, one = np.zeros(len(s)), np.ones(len(s))
        G = [[o, z, -y, one, o, o], [-z, o, x, o, one, o], [y, -x, o, o, o, one]]
        v = np.zeros((len(s), SUMS))
        k = 0
        for i in range(6):
            for j in range(i, 6):
                v[:, k] = (G[0][i] * G[0][j] + G[1][i] * G[1][j]) + G[2][i] * G[2][j]
                k += 1
    v[:, 28] = 1.0
    h, w = lev["D_s"].shape
    tot = ordered_sum(h * w, s, v)
    info = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            info[i, j] = info[j, i] = tot[k]
            k += 1
    return canon64(info)


def is_converged(first, fitness, rmse, prev_fitness, prev_rmse, opt):
    """The convergence rule."""
    return (not first) and abs(fitness - prev_fitness) <= opt.relative_fitness * fitness and \
        abs(rmse - prev_rmse) <= opt.relative_rmse * rmse


ZERO_RECORD = dict(level=0, executed=0, count=0, failed=0, converged=0, e=0.0, A=np.zeros(21), g=np.zeros(6), pose=np.zeros(16))


def compute(pair, opt, levels=None):
    """success, transformation, information, fitness, inlier_rmse, count, iterations, converged_levels and the trace."""
    levels = build_pyramid(pair, opt) if levels is None else levels
    L = len(levels)
    T = np.array(pair.init, dtype=f64)
    T[3] = [0.0, 0.0, 0.0, 1.0]
    trace, failed, count, done, conv_levels, fitness, rmse = [], False, 0, 0, 0, 0.0, 0.0
    for l in range(L - 1, -1, -1):
        lev = levels[l]
        h, w = lev["D_s"].shape
        converged = False
        for k in range(opt.iterations[L - 1 - l]):
            if failed or converged:
                trace.append(dict(ZERO_RECORD))
                continue
            tot = iteration_sums(pair.K, T, l, lev, opt)
            count, done = int(tot[28]), done + 1
            x = solve(tot)
            failed = x is None
            T = np.eye(4) if failed else update(T, x)
            if not failed:
                with np.errstate(all="ignore"):
                    fit, rm = float(count) / float(h * w), float(np.sqrt(f64(tot[27]) / f64(count)))
                converged = is_converged(k == 0, fit, rm, fitness, rmse, opt)
                fitness, rmse = fit, rm
                if converged:
                    conv_levels |= 1 << l
            trace.append(dict(level=l, executed=1, count=count, failed=int(failed), converged=int(converged),
                              e=canon64(tot[27]), A=canon64(tot[:21]), g=canon64(tot[21:27]), pose=T.ravel().copy()))
    info = np.zeros((6, 6)) if failed else information(pair.K, T, levels[0], opt)
    if failed:
        fitness = rmse = 0.0
    return SimpleNamespace(success=int(not failed), transformation=T, information=info, fitness=float(canon64(fitness)),
                           inlier_rmse=float(canon64(rmse)), count=count, iterations=done, converged_levels=conv_levels,
                           trace=trace, levels=levels)


# ---- scenes -----------------------------------------------------------------------------------------------------------
SMALL = O.pose(0.004, -0.006, 0.003, (0.005, -0.003, 0.004))


def make_pair(w, h, motion=SMALL, init=None, depth="u16", pad=0):
    """Source at the identity, target camera at `motion`^-1: the transformation source -> target IS `motion`.  The scene
    is the wall with its balls of tests/odometry_reference.py."""
    K = O.camera(w, h)
    ds, _ = O.render(w, h, K, np.eye(4))
    dt, _ = O.render(w, h, K, np.linalg.inv(motion))
    conv = (lambda d: O.as_uint16(d, pad)) if depth == "u16" else (lambda d: d.astype(f32))
    return SimpleNamespace(K=K, source_depth=conv(ds), target_depth=conv(dt), depth_scale=1000.0,
                           init=np.eye(4) if init is None else np.array(init, dtype=f64), truth=motion)


RECOVERY_MOTION = O.pose(0.012, -0.016, 0.01, (0.015, -0.01, 0.012))


def recovery_pair(w=96, h=72):
    """The scene of the recovery test: the wall with its four spheres, float32 metres.  (One sphere in front of a plane
    would leave the rotation about the plane's normal through the sphere's centre to the silhouette alone.)"""
    return make_pair(w, h, RECOVERY_MOTION, depth="f32")


def pose_error(T, truth):
    """(rotation error in radians, translation error in metres) of T against truth."""
    E = np.linalg.inv(truth) @ T
    return float(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(E[:3, 3]))


_cases = None


def cases():
    """name -> SimpleNamespace(pair, opt, host: also in the host driver's file).  Built once."""
    global _cases
    if _cases is not None:
        return _cases
    c = {}

    def add(name, pair, opt=None, host=True):
        c[name] = SimpleNamespace(name=name, pair=pair, opt=opt or option((3, 2, 2)), host=host)
    one = option((3,))
    # pixel counts at the block edge, one level
    add("block-1", make_pair(17, 15), one)
    add("block", make_pair(16, 16), one)
    add("block+1", make_pair(257, 1, O.pose(t=(0.004, 0.0, 0.0))), one)
    # pixel counts at the group edge (64 blocks of 256 = 128 x 128)
    add("group-1", make_pair(129, 127), option((2,)), host=False)
    add("group", make_pair(128, 128), option((2,)), host=False)
    add("group+1", make_pair(129, 128), option((2,)), host=False)
    # more than eight groups: the finishing kernel's slots wrap (400 x 330 = 516 blocks, 9 groups)
    add("nine_groups", make_pair(400, 330), option((1,)), host=False)
    # the last level is 2 x 1
    add("9x5", make_pair(9, 5), option((2, 2, 2)))
    add("37x29", make_pair(37, 29, pad=3))
    add("64x48", make_pair(64, 48), option((4, 3, 2)), host=False)
    p = make_pair(37, 29, depth="f32")
    for d in (p.source_depth, p.target_depth):
        d[0, 0], d[1, 2], d[2, 1], d[14, 18], d[9, 9] = 0.0, np.nan, -1.0, np.inf, f32(-0.0)
    add("f32_specials", p)
    # an all-invalid source: count 0, the solve fails at the first iteration
    blank = make_pair(37, 29)
    blank.source_depth[:] = 0
    add("all_invalid", blank)
    # identical images at the identity: x = 0, every level converges at its second iteration
    same = make_pair(37, 29, np.eye(4))
    add("converges", same, option((3, 3, 3)))
    # a moving pair: thresholds of 10 are met by any two iterations, a negative one by none (its rmse is not 0)
    add("converges_early", make_pair(37, 29), option((3, 3, 3), relative_rmse=10.0, relative_fitness=10.0))
    add("never_converges", make_pair(37, 29), option((3, 3, 3), relative_rmse=-1.0, relative_fitness=10.0))
    add("skip_level", make_pair(37, 29), option((0, 3)))
    add("no_iteration", make_pair(16, 12, init=O.pose(0.0, 0.01, 0.0, (0.01, 0.0, 0.0))), option((0,)))
    add("depth_range", make_pair(37, 29), option((2, 2), depth_min=1.7, depth_max=1.95))
    add("tight", make_pair(37, 29), option((2, 2), depth_outlier_trunc=0.004, depth_huber_delta=0.001))
    tiny = make_pair(8, 8)
    add("8x8", tiny)
    _cases = c
    return c


_results = {}


def result(name):
    if name not in _results:
        cs = cases()[name]
        _results[name] = compute(cs.pair, cs.opt)
    return _results[name]


def pyramid(name):
    return pyramid_floats(result(name).levels)
