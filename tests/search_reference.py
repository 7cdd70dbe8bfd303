"""Numpy restatement of the neighbour-search contract of include/teaser_hip.h ("Neighbour search"): the stated d2
expression with the query on the left, the (d2, j) order, the strict radius comparison and the row layout of the
uncapped radius search.  The d2 expression and the lexsort are those of tests/outlier_reference.py.  The GPU results are
compared with it for equality; tests/test_search_reference.py pins it against straight loops."""
import numpy as np

import outlier_reference as R


def squared_distances(P, Q, rows):
    """d2[r, j] = ((dx dx + dy dy) + dz dz), dx = Q[rows[r]].x - P[j].x: outlier_reference's expression on the stacked
    cloud [P; Q], whose rows len(P) + rows are the queries and whose first len(P) columns are the data."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    return R.squared_distances(np.concatenate([P, Q]), len(P) + np.asarray(rows))[:, :len(P)]


def _sorted_rows(P, Q, chunk):
    """Per chunk of queries (rows, D, order): order = the data indices in ascending (d2, j)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    jj = np.arange(len(P))
    for lo in range(0, len(Q), chunk):
        rows = np.arange(lo, min(lo + chunk, len(Q)))
        D = squared_distances(P, Q, rows)
        order = np.lexsort((np.broadcast_to(jj, D.shape), D), axis=-1)  # primary key d2, then j
        yield rows, np.take_along_axis(D, order, axis=1), order


def knn_search(P, Q, k, chunk=512):
    """(idx n_query x k int32, d2 n_query x k float64): per query the min(k, n_data) smallest (d2, j), then -1 / +inf."""
    n_q, n_d = len(np.reshape(Q, (-1, 3))), len(np.reshape(P, (-1, 3)))
    m = min(k, n_d)
    idx = np.full((n_q, k), -1, dtype=np.int32)
    d2 = np.full((n_q, k), np.inf)
    for rows, D, order in _sorted_rows(P, Q, chunk):
        idx[rows, :m] = order[:, :m]
        d2[rows, :m] = D[:, :m]
    return idx, d2


def radius_search(P, Q, radius, chunk=512):
    """(idx int32, d2 float64, row_splits int64 n_query + 1): per query every j with d2 < radius radius in ascending
    (d2, j), rows one after the other."""
    n_q = len(np.reshape(Q, (-1, 3)))
    r2 = np.float64(radius) * np.float64(radius)
    idx, d2, counts = [], [], np.zeros(n_q, dtype=np.int64)
    for rows, D, order in _sorted_rows(P, Q, chunk):
        inside = D < r2  # sorted rows: the entries inside are a prefix
        counts[rows] = inside.sum(axis=1)
        idx.append(order[inside])
        d2.append(D[inside])
    splits = np.zeros(n_q + 1, dtype=np.int64)
    np.cumsum(counts, out=splits[1:])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat(idx, np.int32), cat(d2, np.float64), splits


def hybrid_search(P, Q, radius, max_nn, chunk=512):
    """(idx n_query x max_nn int32, d2, count int32): per query the first min(max_nn, number inside) of the radius
    search's row, then -1 / +inf."""
    n_q = len(np.reshape(Q, (-1, 3)))
    r2 = np.float64(radius) * np.float64(radius)
    idx = np.full((n_q, max_nn), -1, dtype=np.int32)
    d2 = np.full((n_q, max_nn), np.inf)
    count = np.zeros(n_q, dtype=np.int32)
    for rows, D, order in _sorted_rows(P, Q, chunk):
        m = min(max_nn, D.shape[1])
        keep = D[:, :m] < r2
        idx[rows, :m] = np.where(keep, order[:, :m], -1)
        d2[rows, :m] = np.where(keep, D[:, :m], np.inf)
        count[rows] = keep.sum(axis=1)
    return idx, d2, count


def lattice(m=7, spacing=0.25):
    """The m^3 dyadic lattice: every d2 between its points, its cell centres and its points is exact."""
    g = spacing * np.arange(m)
    return np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], 1)


def lattice_centres(m=7, spacing=0.25):
    """The (m - 1)^3 cell centres of lattice(m, spacing): eight data points tie at the nearest distance."""
    return lattice(m - 1, spacing) + 0.5 * spacing


# ---- the batch tests/test_gpu_wide_batches.py and tests/test_wide_batch_cases.py share ----
WIDE_KS = (1, 5, 32, 33, 100)
WIDE_TINY = 1e-9  # a radius no query reaches a data point with (the queries are drawn apart from the data)


def wide_batch():
    """320 two-cloud problems: the data are normals_reference.wide_batch()'s clouds (0 .. 65 points), the queries 0 .. 40
    points of the unit cube; dict(data, query, k, radius, hybrid_radius).  The radii are WIDE_TINY in runs of five consecutive problems
    out of every twelve and around problems 255 .. 257, which have entries between neighbours without.  What the wide
    test rests on is asserted from the sizes alone."""
    import normals_reference as RN
    data = RN.wide_batch()
    b = len(data)
    nq = [(7, 40, 0, 1, 33, 12, 20)[i % 7] for i in range(b)]
    for i in (255, 256, 257):
        nq[i] = (9, 33, 2)[i - 255]
    query = [RN.cube(nq[i], 5000 + i) * 1.2 - 0.1 for i in range(b)]
    tiny = [(i % 12 in (2, 3, 4, 5, 6) or 250 <= i <= 262) and i not in (255, 256, 257) for i in range(b)]
    radius = [WIDE_TINY if tiny[i] else (0.3, 0.5, 2.0)[i % 3] for i in range(b)]
    radius[257] = 2.0  # covers the cube: every data point of every query
    k = [WIDE_KS[i % len(WIDE_KS)] for i in range(b)]
    empty = [tiny[i] or len(data[i]) == 0 or nq[i] == 0 for i in range(b)]  # no entry, whatever the points
    assert b > 256 and sum(empty) >= 50
    assert all(empty[i] for i in (250, 251, 252, 253, 254, 258, 259, 260, 261, 262))
    assert not any(tiny[i] for i in (255, 256, 257)) and all(len(data[i]) and nq[i] for i in (255, 256, 257))
    assert any(len(data[i]) == 0 and nq[i] > 0 for i in range(b)) and any(len(data[i]) > 0 and nq[i] == 0 for i in range(b))
    assert sum((n + 255) // 256 for n in nq) > 256  # query blocks
    return dict(data=data, query=query, k=k, radius=radius, hybrid_radius=[(0.3, 0.5, 2.0)[i % 3] for i in range(b)])
