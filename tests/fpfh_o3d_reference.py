"""Numpy restatement of the contract "FPFH (Open3D form)" of include/teaser_hip.h: Open3D's compute_fpfh_feature on given
normals with hybrid or k-NN search, every operation an IEEE double operation in the stated order (numpy's elementwise
ufuncs round once per operation and fuse nothing).  The neighbour lists are those of tests/search_reference.py with the
cloud as its own query set.  The GPU results and the host driver's are compared with it for equality;
tests/test_fpfh_o3d_reference.py pins it against a scalar-loop transcription, hand-checked cases and the libm form."""
import numpy as np

import search_reference as S

HYBRID, KNN = 0, 1
PI = 3.14159265358979323846
DIM = 33


def det_atan(x):
    """|x| <= 1: two argument halvings, then 25 terms of the series, Horner from the last."""
    x = np.asarray(x, dtype=np.float64)
    t = x / (1.0 + np.sqrt(1.0 + x * x))
    t = t / (1.0 + np.sqrt(1.0 + t * t))
    t2 = t * t
    s = np.zeros_like(t)
    for k in range(24, -1, -1):
        s = 1.0 / float(2 * k + 1) - t2 * s
    return 4.0 * (t * s)


def det_atan2(y, x):
    """The deterministic atan2 of csrc/fdet_math.h."""
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    ax, ay = np.abs(x), np.abs(y)
    zero = (x == 0.0) & (y == 0.0)
    big = ax >= ay
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.where(big, ay, ax) / np.where(zero, 1.0, np.where(big, ax, ay))
    a = det_atan(lo)
    a = np.where(big, a, PI / 2 - a)
    a = np.where(x < 0.0, PI - a, a)
    a = np.where(y < 0.0, -a, a)
    return np.where(zero, 0.0, a)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pair_features(p1, n1, p2, n2, atan2=det_atan2, swap=None):
    """(f0, f1, f2, degenerate, swapped) of the pairs (p1, n1), (p2, n2), arrays of shape (..., 3).  atan2 / swap: the
    functions the libm comparison replaces (swap(a1, a2) -> bool; None: |a1| < |a2|)."""
    p1, n1, p2, n2 = (np.asarray(a, dtype=np.float64) for a in (p1, n1, p2, n2))
    dp = p2 - p1
    f3 = np.sqrt(dot(dp, dp))
    deg = f3 == 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a1 = dot(n1, dp) / f3
        a2 = dot(n2, dp) / f3
        sw = (np.abs(a1) < np.abs(a2)) if swap is None else swap(a1, a2)
        sw = sw & ~deg
        s3 = sw[..., None]
        m1, m2 = np.where(s3, n2, n1), np.where(s3, n1, n2)
        dp = np.where(s3, -dp, dp)
        f2 = np.where(sw, -a2, a1)
        v = cross(dp, m1)
        vn = np.sqrt(dot(v, v))
        deg = deg | (vn == 0.0)
        v = v / vn[..., None]
        w = cross(m1, v)
        f1 = dot(v, m2)
        f0 = atan2(dot(w, m2), dot(m1, m2))
    z = np.zeros_like(f3)
    return np.where(deg, z, f0), np.where(deg, z, f1), np.where(deg, z, f2), deg, sw


def clamp_bin(x):
    with np.errstate(invalid="ignore"):
        h = np.floor(x)
        h = np.where(~(h >= 0.0), 0.0, np.where(h > 10.0, 10.0, h))
    return h.astype(np.int64)


def bins(f0, f1, f2):
    """The three bin indices (0..10, 11..21, 22..32)."""
    return (clamp_bin(11.0 * (f0 + PI) / (2.0 * PI)), 11 + clamp_bin(11.0 * (f1 + 1.0) * 0.5),
            22 + clamp_bin(11.0 * (f2 + 1.0) * 0.5))


def neighbour_lists(P, search, radius, max_nn):
    """(idx n x max_nn with -1 behind the valid entries, d2 n x max_nn, m n): the rows of the two-cloud search with the
    cloud as its own query set."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    if search == KNN:
        idx, d2 = S.knn_search(P, P, max_nn)
    elif search == HYBRID:
        idx, d2, _ = S.hybrid_search(P, P, radius, max_nn)
    else:
        raise ValueError("search must be HYBRID or KNN")
    return idx.astype(np.int64), d2, (idx >= 0).sum(axis=1)


def spfh_rows(P, N, idx, m, atan2=det_atan2, swap=None):
    """n x 33 SPFH rows; also the (pairs, 3) bin triples of all valid pairs in (i, k) order."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3)
    n, K = idx.shape
    H = np.zeros((n, DIM))
    triples = []
    if n == 0:
        return H, np.zeros((0, 3), dtype=np.int64)
    with np.errstate(divide="ignore"):
        c = np.where(m > 1, 100.0 / np.maximum(m - 1, 1).astype(np.float64), 0.0)
    rows = np.arange(n)
    for k in range(1, K):
        valid = k < m
        if not valid.any():
            break
        j = np.where(valid, idx[:, k], 0)
        f0, f1, f2, _, _ = pair_features(P, N, P[j], N[j], atan2, swap)
        hs = bins(f0, f1, f2)
        add = np.where(valid, c, 0.0)  # x + 0.0 leaves every x >= 0 as it is
        for h in hs:
            H[rows, h] = H[rows, h] + add
        triples.append((np.flatnonzero(valid), np.stack(hs, 1)[valid]))
    if triples:  # (i, k) order: sort the (k, i) collection by i, stable
        ii = np.concatenate([t[0] for t in triples])
        tt = np.concatenate([t[1] for t in triples])
        tt = tt[np.argsort(ii, kind="stable")]
    else:
        tt = np.zeros((0, 3), dtype=np.int64)
    return H, tt


def fpfh_rows(H, idx, d2, m):
    """n x 33 FPFH rows from the SPFH rows H and the lists."""
    n, K = idx.shape
    F = np.zeros((n, DIM))
    Ssum = np.zeros((n, 3))
    for k in range(1, K):
        valid = (k < m) & (d2[:, k] != 0.0)
        if not (k < m).any():
            break
        j = np.where(valid, idx[:, k], 0)
        den = np.where(valid, d2[:, k], 1.0)
        val = np.where(valid[:, None], H[j] / den[:, None], 0.0)
        for b in range(DIM):
            Ssum[:, b // 11] = Ssum[:, b // 11] + val[:, b]
        F = F + val
    with np.errstate(divide="ignore"):
        scale = np.where(Ssum != 0.0, 100.0 / np.where(Ssum != 0.0, Ssum, 1.0), Ssum)
    F = F * np.repeat(scale, 11, axis=1)
    F = F + H
    F[m <= 1] = 0.0
    return F


def compute_fpfh_feature(P, N, search=HYBRID, radius=0.0, max_nn=100, atan2=det_atan2, swap=None):
    """(fpfh n x 33, spfh n x 33) of the contract."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    if len(P) == 0:
        return np.zeros((0, DIM)), np.zeros((0, DIM))
    idx, d2, m = neighbour_lists(P, search, radius, max_nn)
    H, _ = spfh_rows(P, N, idx, m, atan2, swap)
    return fpfh_rows(H, idx, d2, m), H


# ---- the scalar-loop transcription of the contract (tests/test_fpfh_o3d_reference.py, part 1) --------------------------
def scalar_atan(x):
    t = x / (1.0 + np.sqrt(np.float64(1.0 + x * x)))
    t = t / (1.0 + np.sqrt(np.float64(1.0 + t * t)))
    t2 = t * t
    s = 0.0
    for k in range(24, -1, -1):
        s = 1.0 / float(2 * k + 1) - t2 * s
    return 4.0 * (t * s)


def scalar_atan2(y, x):
    if x == 0.0 and y == 0.0:
        return 0.0
    ax, ay = abs(x), abs(y)
    a = scalar_atan(ay / ax) if ax >= ay else PI / 2 - scalar_atan(ax / ay)
    if x < 0.0:
        a = PI - a
    return -a if y < 0.0 else a


def scalar_pair(p1, n1, p2, n2):
    d3 = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    x3 = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
    p1, n1, p2, n2 = ([float(v) for v in a] for a in (p1, n1, p2, n2))
    dp = [p2[c] - p1[c] for c in range(3)]
    f3 = float(np.sqrt(np.float64(d3(dp, dp))))
    if f3 == 0.0:
        return 0.0, 0.0, 0.0
    a1, a2 = d3(n1, dp) / f3, d3(n2, dp) / f3
    f2 = a1
    if abs(a1) < abs(a2):
        n1, n2 = n2, n1
        dp = [-v for v in dp]
        f2 = -a2
    v = x3(dp, n1)
    vn = float(np.sqrt(np.float64(d3(v, v))))
    if vn == 0.0:
        return 0.0, 0.0, 0.0
    v = [c / vn for c in v]
    w = x3(n1, v)
    return scalar_atan2(d3(w, n2), d3(n1, n2)), d3(v, n2), f2


def scalar_bin(x):
    h = float(np.floor(x))
    return 0 if not h >= 0.0 else (10 if h > 10.0 else int(h))


def scalar_fpfh(P, N, idx, d2, m):
    """(fpfh, spfh) by loops over points, neighbours and bins, exactly as the contract writes them."""
    n = len(P)
    H = np.zeros((n, DIM))
    for i in range(n):
        if m[i] <= 1:
            continue
        c = 100.0 / float(m[i] - 1)
        for k in range(1, m[i]):
            j = idx[i, k]
            f0, f1, f2 = scalar_pair(P[i], N[i], P[j], N[j])
            H[i, scalar_bin(11.0 * (f0 + PI) / (2.0 * PI))] += c
            H[i, 11 + scalar_bin(11.0 * (f1 + 1.0) * 0.5)] += c
            H[i, 22 + scalar_bin(11.0 * (f2 + 1.0) * 0.5)] += c
    F = np.zeros((n, DIM))
    for i in range(n):
        if m[i] <= 1:
            continue
        Ss = [0.0, 0.0, 0.0]
        row = [0.0] * DIM
        for k in range(1, m[i]):
            dk = float(d2[i, k])
            if dk == 0.0:
                continue
            for b in range(DIM):
                val = float(H[idx[i, k], b]) / dk
                Ss[b // 11] += val
                row[b] += val
        for g in range(3):
            if Ss[g] != 0.0:
                Ss[g] = 100.0 / Ss[g]
        for b in range(DIM):
            t = row[b] * Ss[b // 11]
            F[i, b] = t + float(H[i, b])
    return F, H


# ---- the clouds the tests share -------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_cloud(n, seed):
    """n points in the unit cube with random unit normals."""
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)), (unit(rng.normal(size=(n, 3))) if n else np.zeros((0, 3)))


def axis_lattice(m=4, spacing=0.25):
    """The m^3 dyadic lattice with normals along the axes (cycling x, y, z, -x, -y, -z by index): exact ties in (d2, j),
    exact a1 == a2, and pairs with dp parallel to n1 (degenerate)."""
    P = S.lattice(m, spacing)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=np.float64)
    return P, axes[np.arange(len(P)) % 6]


def case_list():
    """(name, points, normals, search, radius, max_nn): the cases the host driver and the GPU test share."""
    rng = np.random.default_rng(11)
    out = []
    for n in (0, 1, 2, 63, 64, 65, 257):
        P, N = random_cloud(n, 100 + n)
        out.append(("n%d" % n, P, N, HYBRID if n % 2 else KNN, 0.3, 10))
    P, N = axis_lattice(4)
    out.append(("lattice_hybrid", P, N, HYBRID, 0.3, 20))
    out.append(("lattice_knn", P, N, KNN, 0.0, 27))
    P, N = random_cloud(90, 5)
    P[20:50] = P[60]  # coincident points: position 0 of point 60's list is point 20
    out.append(("duplicates", P, N, HYBRID, 0.25, 40))
    P, N = random_cloud(70, 6)
    out.append(("shifted", P + 1e4, N, HYBRID, 0.35, 15))
    P, N = random_cloud(300, 7)
    out.append(("max_nn_2", 0.3 * P, N, HYBRID, 0.3, 2))
    out.append(("max_nn_100", 0.3 * P, N, HYBRID, 0.3, 100))  # far more than 100 points inside the radius
    out.append(("isolated", P, N, HYBRID, 1e-3, 30))
    P, N = random_cloud(17, 8)
    out.append(("knn_n_below_max_nn", P, N, KNN, 0.0, 50))
    out.append(("knn_100", rng.random((130, 3)), unit(rng.normal(size=(130, 3))), KNN, 0.0, 100))
    return out


def wide_batch():
    """320 clouds of 0 .. 65 points (normals_reference.wide_batch()) with random unit normals, the searches hybrid and
    k-NN in turn: a list of (points, normals, search, radius, max_nn).  It serves FPFH and boundary detection.  What
    the wide tests rest on is asserted from the sizes alone."""
    import normals_reference as RN
    clouds = RN.wide_batch()
    b = len(clouds)
    out = []
    for i, P in enumerate(clouds):
        rng = np.random.default_rng(8000 + i)
        N = unit(rng.normal(size=P.shape)) if len(P) else np.zeros((0, 3))
        if (i // 8 + i) % 2:
            out.append((P, N, HYBRID, (0.3, 0.5)[i % 2], (10, 40)[(i // 2) % 2]))
        else:
            out.append((P, N, KNN, 0.0, (5, 33, 12)[i % 3]))
    assert b > 256
    for search in (HYBRID, KNN):  # each of the two concatenated block lists: a block or more per non-empty cloud
        assert sum(1 for c in out if c[2] == search and len(c[0])) > 128
    assert {out[i][2] for i in (255, 256, 257)} == {HYBRID, KNN}
    return out
