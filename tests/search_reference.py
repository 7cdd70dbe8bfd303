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
