"""Numpy restatement of the normals contract of include/teaser_hip.h ("Normal estimation"), built on the pieces the
covariance and self k-NN contracts are already pinned with: icp_gicp_reference.neighbourhood / sample_covariance /
jacobi3 and outlier_reference.self_knn.  It adds what is new: the eigenvalue order, the choice of the normal and the
three orientation rules with their fill-ins for a zero normal."""
import numpy as np
from scipy.spatial import cKDTree

import icp_gicp_reference as RG
import outlier_reference as RO

HYBRID, KNN = 0, 1


def ascending3(a, b, c):
    """The contract's three exchanges (equal to a sort for numbers; written out so that the bits are by construction)."""
    if b < a:
        a, b = b, a
    if c < b:
        b, c = c, b
    if b < a:
        a, b = b, a
    return a, b, c


def neighbours(P, search, radius, max_nn):
    """Per point the neighbour indices in ascending (d2, j)."""
    n = len(P)
    if search == KNN:
        idx, _ = RO.self_knn(P, max_nn)
        m = min(max_nn, n)
        return [idx[i, :m].astype(np.int64) for i in range(n)]
    tree = cKDTree(P)
    return [RG.neighbourhood(P, i, radius, max_nn, tree)[0] for i in range(n)]


def orient(nrm, p, mode, ref):
    """One normal (zero: fewer than three neighbours) through the orientation step."""
    ref = np.asarray(ref, dtype=np.float64)
    if not nrm.any():
        if mode == 1:
            v = ref - p
            ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            return np.array([0.0, 0.0, 1.0]) if ln == 0 else v / ln
        if mode == 2:
            return ref.copy()
        return np.array([0.0, 0.0, 1.0])
    if mode == 1:
        v = ref - p
        dot = (nrm[0] * v[0] + nrm[1] * v[1]) + nrm[2] * v[2]
    elif mode == 2:
        dot = (nrm[0] * ref[0] + nrm[1] * ref[1]) + nrm[2] * ref[2]
    else:
        dot = 0.0
    return -nrm if dot < 0 else nrm


def estimate_normals(points, search=HYBRID, radius=0.0, max_nn=30, orient_mode=0, ref=(0.0, 0.0, 0.0), order=None):
    """(normals n x 3, raw covariances n x 3 x 3, ascending eigenvalues n x 3, neighbour counts n).  order: None, or a
    function js -> js that reorders a neighbour list before the sums (the shuffled-order experiment of the tests)."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    N, Cv, E, M = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    if n == 0:
        return N, Cv, E, M
    nb = neighbours(P, search, radius, max_nn)
    for i in range(n):
        js = nb[i]
        M[i] = len(js)
        v = np.zeros(3)
        if len(js) >= 3:
            a = RG.sample_covariance(P, i, js if order is None else order(js))
            Cv[i] = [[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]]
            diag, V = RG.jacobi3(a)
            k = 0
            if diag[1] < diag[k]:
                k = 1
            if diag[2] < diag[k]:
                k = 2
            v = V[:, k]
            v = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            E[i] = ascending3(diag[0], diag[1], diag[2])
        N[i] = orient(v, P[i], orient_mode, ref)
    return N, Cv, E, M


def normal_bar(E, c=512.0):
    """The per-point bar on |n_gpu - n_ref| of tests/test_gpu_icp_gicp.py's covariances: c 2^-52 lambda2 /
    (lambda1 - lambda0); inf where the two smallest eigenvalues tie."""
    with np.errstate(divide="ignore", invalid="ignore"):
        bar = c * 2.0 ** -52 * E[:, 2] / (E[:, 1] - E[:, 0])
    return np.where(E[:, 1] > E[:, 0], bar, np.inf)


def surface_variation(E):
    s = (E[:, 0] + E[:, 1]) + E[:, 2]
    out = np.zeros(len(E))
    np.divide(E[:, 0], s, out=out, where=s != 0)
    return out


# ---- the clouds the tests share -------------------------------------------------------------------------------------
def cube(n, seed=3):
    return np.random.default_rng(seed).random((n, 3))


def planar(n=129, seed=4):
    """z = 0 sampled on a jittered grid: every neighbourhood's covariance has a zero row and column, lambda0 = 0."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(np.sqrt(n)))
    g = np.stack([a.ravel() for a in np.meshgrid(np.arange(k), np.arange(k), indexing="ij")], 1)[:n].astype(np.float64)
    g += 0.3 * rng.random(g.shape)
    return np.concatenate([0.1 * g, np.zeros((n, 1))], 1)


def collinear(n=65):
    t = 0.125 * np.arange(n, dtype=np.float64)
    return np.stack([t, 2 * t, -0.5 * t], 1)


def identical(n=64):
    return np.tile([[0.3, -1.25, 7.0]], (n, 1))


def tied_lattice():
    """5 x 5 x 5 lattice with spacing 1/4: every coordinate and every d2 exact, so neighbours tie exactly."""
    g = 0.25 * np.arange(5.0)
    return np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], 1)


WIDE_BATCH = 320
WIDE_CYCLE = (0, 1, 2, 5, 33, 64, 65, 40)
WIDE_ROTATE = 4  # cloud i has WIDE_CYCLE[(i + 4) % 8] points: 255, 256, 257 -> 5, 33, 64; 260 -> 0; 319 -> 5


def wide_batch():
    """320 small clouds for the calls that need more than 256 clouds and more than 256 point blocks
    (tests/test_gpu_batch_width.py), with what those tests rest on asserted from the sizes alone."""
    b = WIDE_BATCH
    n = [WIDE_CYCLE[(i + WIDE_ROTATE) % len(WIDE_CYCLE)] for i in range(b)]
    assert b > 256
    assert sum((k + 255) // 256 for k in n) >= 257  # point blocks: thread 256 of the per-block kernels has work
    assert all(n[i] > 0 for i in (255, 256, 257)) and len({n[255], n[256], n[257]}) == 3
    assert any(n[i] == 0 for i in range(257, b)) and n[b - 1] > 0 and n[0] > 0
    return [cube(n[i], 1000 + i) for i in range(b)]
