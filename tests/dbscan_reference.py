"""The numpy restatement of DBSCAN clustering (include/teaser_hip.h, "DBSCAN clustering"): Open3D's
PointCloud.cluster_dbscan in closed form, a literal copy of its loop with a caller-given pop order, and the scenes the
tests share.  No grid anywhere: the neighbour sets are blocked brute force, so the device's walk over the sorted cell
index is checked against an independent neighbour set.  Every scene lies on integer or dyadic coordinates, so that d2 is
exact and a pair at d2 == eps^2 is a pair at d2 == eps^2 on every machine."""
import functools

import numpy as np


def neighbours(P, eps, block=512):
    """The n x n boolean matrix of d2(i, j) < eps * eps, d2 = (e0*e0 + e1*e1) + e2*e2 in FP64 (numpy contracts
    nothing)."""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    r2 = np.float64(eps) * np.float64(eps)
    A = np.zeros((n, n), dtype=bool)
    for lo in range(0, n, block):
        e = P[lo:lo + block, None, :] - P[None, :, :]
        e0, e1, e2 = e[..., 0], e[..., 1], e[..., 2]
        A[lo:lo + block] = ((e0 * e0 + e1 * e1) + e2 * e2) < r2
    return A


def dbscan(P, eps, min_points, A=None):
    """The closed form: (labels, counts, roots, c), int32 arrays of length n and the number of clusters."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    labels = np.full(n, -1, dtype=np.int32)
    roots = np.full(n, -1, dtype=np.int32)
    if n == 0 or not (np.float64(eps) * np.float64(eps) > 0):
        return labels, np.zeros(n, dtype=np.int32), roots, 0
    if A is None:
        A = neighbours(P, eps)
    counts = A.sum(axis=1).astype(np.int32)
    core = counts >= min_points
    c = 0
    for i in range(n):  # ascending: a component is opened at its smallest core index
        if not core[i] or roots[i] >= 0:
            continue
        roots[i] = i
        labels[i] = c
        stack = [i]
        while stack:
            u = stack.pop()
            for v in np.flatnonzero(A[u] & core & (roots < 0)):
                roots[v] = i
                labels[v] = c
                stack.append(int(v))
        c += 1
    for i in np.flatnonzero(~core):
        nb = np.flatnonzero(A[i] & core)
        if len(nb):
            labels[i] = labels[nb].min()
    return labels, counts, roots, c


def dbscan_literal(P, eps, min_points, rng, A=None):
    """Open3D's ClusterDBSCAN loop, statement for statement, with the pop order of its unordered_set drawn from rng.
    Returns the labels."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    if A is None:
        A = neighbours(P, eps) if np.float64(eps) * np.float64(eps) > 0 else np.zeros((n, n), dtype=bool)
    nbs = [np.flatnonzero(A[i]).tolist() for i in range(n)]
    labels = [-2] * n
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if len(nbs[idx]) < min_points:
            labels[idx] = -1
            continue
        nbs_next = set(nbs[idx])
        visited = {idx}
        labels[idx] = cluster
        while nbs_next:
            pool = sorted(nbs_next)
            nb = pool[int(rng.integers(len(pool)))]
            nbs_next.discard(nb)
            visited.add(nb)
            if labels[nb] == -1:
                labels[nb] = cluster
            if labels[nb] != -2:
                continue
            labels[nb] = cluster
            if len(nbs[nb]) >= min_points:
                for q in nbs[nb]:
                    if q not in visited:
                        nbs_next.add(q)
        cluster += 1
    return np.array(labels, dtype=np.int32).reshape(n)


# ---- scenes: (points, eps, min_points) -------------------------------------------------------------------------------

def lattice_slab(nx=9, ny=7, nz=3, spacing=0.25, seed=1):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    P = g.astype(np.float64) * spacing
    return P[np.random.default_rng(seed).permutation(len(P))]


def random_lattice(rng, n, side=6, spacing=0.5):
    return rng.integers(0, side, size=(n, 3)).astype(np.float64) * spacing


def contested(b_first=False):
    """Two rows of 10 points (spacing 0.5) that end 3 apart, and one point c half-way between their ends.  With
    eps = 1.75 and min_points = 4 every row point is core (an end point sees 4 row points), c sees itself and the two
    ends (3: not core) and is a border point of BOTH clusters: the cluster of smaller number must win.
    b_first=False: indices [c, A0..A9, B0..B9]: c is visited first, as noise, and relabelled.  Expected labels
    [0, 0 x 10, 1 x 10], roots [-1, 1 x 10, 11 x 10].
    b_first=True: indices [B0..B9, A0..A9, c].  Expected labels [0 x 10, 1 x 10, 0], roots [0 x 10, 10 x 10, -1]."""
    k = np.arange(10, dtype=np.float64)
    A = np.stack([-0.5 * k, 0 * k, 0 * k], 1)
    B = np.stack([3.0 + 0.5 * k, 0 * k, 0 * k], 1)
    c = np.array([[1.5, 0.0, 0.0]])
    P = np.concatenate([B, A, c] if b_first else [c, A, B])
    return P, 1.75, 4


def contested_expected(b_first=False):
    if b_first:
        labels = [0] * 10 + [1] * 10 + [0]
        roots = [0] * 10 + [10] * 10 + [-1]
        counts = [5, 5, 6, 7, 7, 7, 7, 6, 5, 4] * 2 + [3]
    else:
        labels = [0] + [0] * 10 + [1] * 10
        roots = [-1] + [1] * 10 + [11] * 10
        counts = [3] + [5, 5, 6, 7, 7, 7, 7, 6, 5, 4] * 2
    return np.array(labels, np.int32), np.array(counts, np.int32), np.array(roots, np.int32), 2


def touching(joined=False):
    """Two blobs of five points whose closest pairs lie at exactly d2 == 1.  eps = 1: strict <, NOT joined (2 clusters of
    5).  eps = nextafter(1, inf): eps * eps = 1 + 2^-51 > 1, joined (1 cluster of 10).  min_points = 3."""
    A = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25], [0.25, 0.25, 0]], dtype=np.float64)
    P = np.concatenate([A, A + np.array([1.25, 0.0, 0.0])])
    return P, (np.nextafter(1.0, np.inf) if joined else 1.0), 3


CHAIN_N = 4097


def chain(order="ascending", n=CHAIN_N):
    """n points spaced 0.75 eps on a line (eps = 1): each sees itself and its two chain neighbours.  min_points = 2:
    one cluster, root = the index of the smallest label holder, a union-find path as long as the chain."""
    x = 0.75 * np.arange(n, dtype=np.float64)
    if order == "descending":
        x = x[::-1]
    elif order == "shuffled":
        x = x[np.random.default_rng(4097).permutation(n)]
    else:
        assert order == "ascending"
    P = np.stack([x, np.zeros(n), np.zeros(n)], 1)
    return np.ascontiguousarray(P), 1.0, 2


def comb(m=2040):
    """Two chains (y = 0 and y = 8.25, x = 0 .. 0.75 m) joined only at their far ends by a chain along y: indices run
    from the near end of the first chain, then from the near end of the second, the connector last, so the two trees
    grow apart and meet through the last points."""
    k = np.arange(m + 1, dtype=np.float64)
    c1 = np.stack([0.75 * k, 0 * k, 0 * k], 1)
    c2 = np.stack([0.75 * k, 0 * k + 8.25, 0 * k], 1)
    j = np.arange(1, 11, dtype=np.float64)
    con = np.stack([0 * j + 0.75 * m, 0.75 * j, 0 * j], 1)
    return np.concatenate([c1, c2, con]), 1.0, 2


def identical(n=513):
    return np.tile(np.array([[0.5, 0.25, -1.0]]), (n, 1)), 0.5, 4


def shifted():
    return lattice_slab(8, 8, 4, 0.25, seed=3) + np.array([1e6, -1e6, 1e6]), 0.3, 5


def flat(n=600, seed=5):
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 3))
    P[:, :2] = rng.integers(0, 64, size=(n, 2)) / 8.0
    return P, 0.5, 4


def diagonal(n=300):
    """A line along (1, 1, 1), spacing 0.5 per axis: with eps = 1 one cluster that crosses a cell boundary on all three
    axes at every other point."""
    k = 0.5 * np.arange(n, dtype=np.float64)
    P = np.stack([k, k, k], 1)
    return P[np.random.default_rng(7).permutation(n)], 1.0, 3


def builders():
    """name -> (points, eps, min_points): every scene of the issue's list."""
    out = {"slab": (lattice_slab(), 0.3, 5), "slab_wide": (lattice_slab(), 0.51, 12),
           "contested": contested(False), "contested_b_first": contested(True),
           "touching": touching(False), "touching_joined": touching(True),
           "chain_ascending": chain("ascending"), "chain_descending": chain("descending"),
           "chain_shuffled": chain("shuffled"), "comb": comb(), "identical": identical(), "shifted": shifted(),
           "flat": flat(), "diagonal": diagonal()}
    return out


@functools.lru_cache(maxsize=None)
def adjacency(name):
    """The neighbour matrix of a builder's scene, computed once and shared (read-only)."""
    P, eps, _ = builders()[name]
    A = neighbours(P, eps)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def expected(name, min_points=None):
    """dbscan() of a builder's scene (min_points: the scene's own unless given), computed once and shared."""
    P, eps, mp = builders()[name]
    out = dbscan(P, eps, mp if min_points is None else min_points, adjacency(name))
    for a in out[:3]:
        a.setflags(write=False)
    return out


def wide_batch():
    """normals_reference.wide_batch()'s 320 clouds of 0 .. 65 points with eps and min_points in turn: (clouds, eps,
    min_points).  What the wide test rests on (more than 256 clouds and more than 256 point blocks) is asserted there
    from the sizes alone."""
    import normals_reference as RN
    clouds = RN.wide_batch()
    b = len(clouds)
    eps = [(0.15, 0.3, 0.6)[i % 3] for i in range(b)]
    min_points = [(1, 3, 6)[(i // 3) % 3] for i in range(b)]
    assert len({(eps[i], min_points[i]) for i in range(b)}) == 9  # every pairing of the two cycles
    return clouds, eps, min_points
