"""Numpy restatement of the contract "Boundary points" of include/teaser_hip.h: Open3D's compute_boundary_points (the
angle criterion of PCL's BoundaryEstimation), every operation an IEEE double operation in the stated order (numpy's
elementwise ufuncs round once per operation and fuse nothing).  The neighbour lists are those of the FPFH restatement
(tests/fpfh_o3d_reference.py).  The GPU results and the host driver's are compared with it for equality.  A second,
scalar form written independently (plain Python loops, a successor search instead of a sort) is held against it bit for
bit by tests/test_boundary_reference.py, beside analytic cases."""
import math

import numpy as np

from fpfh_o3d_reference import HYBRID, KNN, PI, cross, det_atan2, dot, neighbour_lists, scalar_atan2  # noqa: F401


def frames(N):
    """(u, v, ok) of the normals N (n x 3): Eigen's unitOrthogonal and cross(n, v); ok: every component finite."""
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    ax, ay, az = np.abs(N[:, 0]), np.abs(N[:, 1]), np.abs(N[:, 2])
    first = ~(ax <= 1e-12 * az) | ~(ay <= 1e-12 * az)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s1 = 1.0 / np.sqrt(N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1])
        s2 = 1.0 / np.sqrt(N[:, 1] * N[:, 1] + N[:, 2] * N[:, 2])
        z = np.zeros(len(N))
        v1 = np.stack([-N[:, 1] * s1, N[:, 0] * s1, z], 1)
        v2 = np.stack([z, -N[:, 2] * s2, N[:, 1] * s2], 1)
        v = np.where(first[:, None], v1, v2)
        u = cross(N, v)
    ok = np.isfinite(u).all(axis=1) & np.isfinite(v).all(axis=1)
    return u, v, ok


def max_gaps(P, N, idx, m, atan2=det_atan2):
    """max_gap (n doubles) of the contract from the lists (idx n x K with -1 behind the m valid entries)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n, K = idx.shape
    u, v, ok = frames(N)
    A = np.full((n, max(K - 1, 1)), np.inf)
    for k in range(1, K):
        valid = k < m
        if not valid.any():
            break
        j = np.where(valid, idx[:, k], 0)
        delta = P[j] - P
        with np.errstate(invalid="ignore", over="ignore"):
            a = atan2(dot(v, delta), dot(u, delta))
        a = np.where((delta == 0.0).all(axis=1), 0.0, a)
        A[:, k - 1] = np.where(valid, a, np.inf)
    gap = np.zeros(n)
    for i in range(n):
        cnt = int(m[i]) - 1
        if not ok[i]:
            gap[i] = np.nan
            continue
        if cnt < 1:
            continue
        a = A[i, :cnt]
        if np.isnan(a).any():
            gap[i] = np.nan
            continue
        a = np.sort(a)
        g = 0.0
        d = a[1:] - a[:-1]
        for t in range(cnt - 1):
            if d[t] > g:
                g = d[t]
        w = (2.0 * PI - a[-1]) + a[0]
        if w > g:
            g = w
        gap[i] = g
    return gap


def boundary_points(P, N, search=HYBRID, radius=0.0, max_nn=30, angle_threshold=90.0, atan2=det_atan2):
    """(mask n bools, max_gap n doubles, m n int32) of the contract."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    if len(P) == 0:
        return np.zeros(0, dtype=bool), np.zeros(0), np.zeros(0, dtype=np.int32)
    idx, _, m = neighbour_lists(P, search, radius, max_nn)
    gap = max_gaps(P, N, idx, m, atan2)
    with np.errstate(invalid="ignore"):
        mask = gap > (np.float64(angle_threshold) * PI) / 180.0
    return mask, gap, m.astype(np.int32)


# ---- the second form: scalar loops, a successor search instead of a sort ----------------------------------------------
def scalar_boundary(P, N, idx, m, angle_threshold):
    """(mask, max_gap) by plain Python loops.  For every angle its successor on the circle is looked for directly: the
    smallest angle above it (or an equal one later in the list, so that ties form a chain), else the wrap to the
    smallest angle of all.  The gaps formed are those of consecutive sorted angles and the wrap term, so the largest is
    the contract's max_gap."""
    P = [[float(c) for c in p] for p in np.asarray(P, dtype=np.float64).reshape(-1, 3)]
    N = [[float(c) for c in p] for p in np.asarray(N, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    thr = (float(angle_threshold) * PI) / 180.0
    mask, gaps = [False] * n, [0.0] * n
    for i in range(n):
        nx, ny, nz = N[i]
        if not (abs(nx) <= 1e-12 * abs(nz)) or not (abs(ny) <= 1e-12 * abs(nz)):
            q = nx * nx + ny * ny
            s = 1.0 / math.sqrt(q) if q > 0.0 else math.inf
            v = [-ny * s, nx * s, 0.0]
        else:
            q = ny * ny + nz * nz
            s = 1.0 / math.sqrt(q) if q > 0.0 else (math.inf if q == 0.0 else math.nan)
            v = [0.0, -nz * s, ny * s]
        u = [ny * v[2] - nz * v[1], nz * v[0] - nx * v[2], nx * v[1] - ny * v[0]]
        if not all(math.isfinite(c) for c in u + v):
            gaps[i] = math.nan
            continue
        if m[i] <= 1:
            continue
        ang = []
        for k in range(1, int(m[i])):
            pj = P[int(idx[i][k])]
            d = [pj[0] - P[i][0], pj[1] - P[i][1], pj[2] - P[i][2]]
            if d[0] == 0.0 and d[1] == 0.0 and d[2] == 0.0:
                ang.append(0.0)
            else:
                ang.append(float(scalar_atan2((v[0] * d[0] + v[1] * d[1]) + v[2] * d[2],
                                              (u[0] * d[0] + u[1] * d[1]) + u[2] * d[2])))
        if any(math.isnan(a) for a in ang):
            gaps[i] = math.nan
            continue
        lo = min(range(len(ang)), key=lambda t: (ang[t], t))
        best = 0.0
        for t, a in enumerate(ang):
            succ = None  # the next angle in the order (value, position)
            for w, b in enumerate(ang):
                if (b, w) > (a, t) and (succ is None or (b, w) < (ang[succ], succ)):
                    succ = w
            d = ang[succ] - a if succ is not None else (2.0 * PI - a) + ang[lo]
            if d > best:
                best = d
        gaps[i] = best
        mask[i] = best > thr
    return np.array(mask, dtype=bool), np.array(gaps, dtype=np.float64)


# ---- the clouds the tests share -------------------------------------------------------------------------------------
def plane_lattice(side=9, spacing=0.125, normal="z"):
    """side x side points in a plane (dyadic spacing: exact coordinates) with the constant normal +z or +x."""
    g = np.arange(side, dtype=np.float64) * spacing
    a, b = np.meshgrid(g, g, indexing="ij")
    z = np.zeros(side * side)
    if normal == "z":
        P, nrm = np.stack([a.ravel(), b.ravel(), z], 1), [0.0, 0.0, 1.0]
    else:
        P, nrm = np.stack([z, a.ravel(), b.ravel()], 1), [1.0, 0.0, 0.0]
    return np.ascontiguousarray(P), np.tile(np.array(nrm), (len(P), 1))


def lattice_perimeter(side=9):
    a, b = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    return ((a == 0) | (a == side - 1) | (b == 0) | (b == side - 1)).ravel()


def fibonacci_sphere(n=400):
    """n points on the unit sphere (the golden-angle spiral) with radial normals."""
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    P = np.ascontiguousarray(np.stack([r * np.cos(phi), r * np.sin(phi), z], 1))
    return P, P.copy()


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    P = rng.random((n, 3))
    N = rng.normal(size=(n, 3))
    return P, (N / np.linalg.norm(N, axis=1, keepdims=True) if n else np.zeros((0, 3)))


def case_list():
    """(name, points, normals, search, radius, max_nn, angle_threshold): the cases the host driver and the GPU test
    share."""
    out = []
    P, N = plane_lattice(9, 0.125, "z")
    out.append(("lattice_z", P, N, HYBRID, 1.5 * 0.125, 30, 90.0))
    P, N = plane_lattice(9, 0.125, "x")
    out.append(("lattice_x", P, N, HYBRID, 1.5 * 0.125, 30, 90.0))
    P, N = fibonacci_sphere(400)
    out.append(("sphere", P, N, HYBRID, 0.35, 30, 90.0))
    keep = P[:, 2] >= 0.0
    out.append(("hemisphere", np.ascontiguousarray(P[keep]), np.ascontiguousarray(N[keep]), HYBRID, 0.35, 30, 90.0))
    P, N = random_cloud(257, 357)
    out.append(("n257", P, N, HYBRID, 0.3, 10, 90.0))
    out.append(("n257_full", P, N, HYBRID, 2.0, 100, 60.0))  # every list is full: 99 angles, both slots of every lane
    for k in (2, 33, 64, 65):  # the lane-slot edges
        out.append(("knn%d" % k, P, N, KNN, 0.0, k, 90.0))
    for n in (0, 1, 2, 63, 64, 65):
        Q, M = random_cloud(n, 100 + n)
        out.append(("n%d" % n, Q, M, HYBRID if n % 2 else KNN, 0.4, 12, 45.0))
    P, N = random_cloud(90, 5)
    P[20:50] = P[60]  # coincident points: angle 0.0, and position 0 of point 60's list is point 20
    out.append(("duplicates", P, N, HYBRID, 0.25, 40, 90.0))
    P, N = random_cloud(70, 6)
    N = N.copy()
    N[3] = 0.0                      # no tangent frame: NaN gap
    N[4] = [0.0, 0.0, 1.0]          # the second frame branch
    N[5] = [1e-13, 0.0, 1.0]        # still the second branch
    N[6] = [1e-11, 0.0, 1.0]        # the first
    N[7] = [0.0, 0.0, -2.5]         # not normalised, second branch
    N[8] = [1e200, 1e200, 0.0]      # the squares overflow: s = 0, v = 0, still finite
    out.append(("frames", P, N, HYBRID, 0.4, 20, 120.0))
    P, N = random_cloud(80, 7)
    out.append(("isolated", P, N, HYBRID, 1e-3, 30, 90.0))
    out.append(("threshold_0", P, N, KNN, 0.0, 9, 0.0))
    out.append(("threshold_360", P, N, KNN, 0.0, 3, 360.0))
    out.append(("shifted", P + 1e4, N, HYBRID, 0.35, 15, 90.0))
    return out
