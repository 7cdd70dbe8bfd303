"""Numpy restatement of the self k-NN and outlier-removal contracts of include/teaser_hip.h ("Self k-NN", "Outlier
removal"): the stated d2 expression, the (d2, j) order, the one-term-at-a-time sums and the 256-block reduction.  The
GPU results are compared with it bit for bit; tests/test_outlier_reference.py pins it against straight loops."""
import numpy as np

BLOCK = 256


def squared_distances(P, rows):
    """d2[r, j] = ((dx dx + dy dy) + dz dz), dx = P[rows[r]].x - P[j].x: every product and sum rounded on its own."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    dx = P[rows, 0][:, None] - P[None, :, 0]
    dy = P[rows, 1][:, None] - P[None, :, 1]
    dz = P[rows, 2][:, None] - P[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def self_knn(P, k, chunk=512):
    """(idx n x k int32, d2 n x k float64): per point the min(k, n) smallest (d2, j), then -1 / +inf."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    m = min(k, n)
    idx = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf)
    jj = np.arange(n)
    for lo in range(0, n, chunk):
        rows = np.arange(lo, min(lo + chunk, n))
        D = squared_distances(P, rows)
        order = np.lexsort((np.broadcast_to(jj, D.shape), D), axis=-1)[:, :m]  # primary key d2, then j
        idx[rows, :m] = order
        d2[rows, :m] = np.take_along_axis(D, order, axis=1)
    return idx, d2


def block_sum(terms, use):
    """The contract's SUM of terms[use]: inside each block of 256 consecutive indices in ascending index from 0.0, then
    the block sums in ascending block order from 0.0.  (Adding +0.0 for an unused point leaves a non-negative running
    sum's bits alone, which lets the inner loop run over the blocks side by side.)"""
    n = len(terms)
    nb = (n + BLOCK - 1) // BLOCK
    t = np.zeros(nb * BLOCK)
    t[:n] = np.where(use, terms, 0.0)
    t = t.reshape(nb, BLOCK)
    s = np.zeros(nb)
    for c in range(BLOCK):
        s = s + t[:, c]
    total = 0.0
    for b in range(nb):
        total = total + s[b]
    return np.float64(total)


def statistical(P, nb_neighbors, std_ratio):
    """dict(keep uint8 n, avg n, mean, std, threshold) of remove_statistical_outlier."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    if n == 0:
        return dict(keep=np.zeros(0, dtype=np.uint8), avg=np.zeros(0), mean=np.nan, std=np.nan, threshold=np.nan)
    m = min(nb_neighbors, n)
    _, d2 = self_knn(P, nb_neighbors)
    acc = np.zeros(n)
    for t in range(m):  # one term at a time in ascending (d2, j), from 0.0
        acc = acc + np.sqrt(d2[:, t])
    avg = acc / np.float64(m)
    use = avg > 0
    valid = np.float64(n)
    with np.errstate(all="ignore"):
        mean = block_sum(avg, use) / valid
        e = avg - mean
        std = np.sqrt(block_sum(e * e, use) / (valid - np.float64(1.0)))
        threshold = mean + np.float64(std_ratio) * std
        keep = (use & (avg < threshold)).astype(np.uint8)
    return dict(keep=keep, avg=avg, mean=mean, std=std, threshold=threshold)


def radius(P, nb_points, r, chunk=512):
    """dict(keep uint8 n, count int32 n) of remove_radius_outlier: count of j (i included) with d2 < r r."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    count = np.zeros(n, dtype=np.int32)
    r2 = np.float64(r) * np.float64(r)
    for lo in range(0, n, chunk):
        rows = np.arange(lo, min(lo + chunk, n))
        count[rows] = (squared_distances(P, rows) < r2).sum(axis=1)
    return dict(keep=(count > nb_points).astype(np.uint8), count=count)


def planted_cloud(seed=5, n=600, planted=6):
    """A seeded cloud for the statistical rule: n points uniform in the unit cube and `planted` points far outside it
    (8 to 13 cube edges away along the diagonal, one edge apart from each other), placed at seeded positions of the
    index range.  Returns (points, the sorted planted indices)."""
    rng = np.random.default_rng(seed)
    P = rng.random((n + planted, 3))
    where = np.sort(rng.choice(n + planted, size=planted, replace=False))
    for t, i in enumerate(where):
        P[i] = (8.0 + t) * np.ones(3) + 0.01 * rng.random(3)
    return P, where


def bits_equal(a, b):
    """Equal bits, with one exception: NaN equals NaN (0 / 0 has its sign bit set on x86 and clear on the GPU, and the
    contract only says NaN)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
