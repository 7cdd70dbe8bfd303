"""numpy restatement of the k-nearest-neighbour semantics of include/teaser_hip.h ("k nearest"): the reference the GPU
tests compare with, exactly.  Distances are accumulated one dimension at a time in numpy float32 arrays -- every
subtraction, product and sum rounded to IEEE single, nothing fused -- and the k nearest are the first
k_eff = min(k, n_data) finite candidates of np.lexsort((index, d)): ascending d, ties to the lower index."""
import numpy as np


def sq_distances(query, data):
    """n_query x n_data float32: d = 0; for c in 0 .. dim-1: t = q_c - x_c; d += t * t."""
    q, x = np.asarray(query, dtype=np.float32), np.asarray(data, dtype=np.float32)
    d = np.zeros((q.shape[0], x.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(q.shape[1] if q.ndim == 2 else 0):
            t = q[:, c][:, None] - x[:, c][None, :]
            d = d + t * t
    assert d.dtype == np.float32
    return d


def knn(data, query, k):
    """(idx n_query x k int32, dist n_query x k float32): slots beyond k_eff hold -1 / +inf.  NaN and +inf distances
    never enter a list; a query left with fewer than k_eff entries raises ValueError (non-finite features)."""
    data, query = np.asarray(data, dtype=np.float32), np.asarray(query, dtype=np.float32)
    nd, nq = data.shape[0], query.shape[0]
    idx = np.full((nq, k), -1, dtype=np.int32)
    dist = np.full((nq, k), np.inf, dtype=np.float32)
    if nd == 0 or nq == 0:
        return idx, dist
    d = sq_distances(query, data)
    k_eff = min(k, nd)
    index = np.arange(nd)
    for q in range(nq):
        order = np.lexsort((index, d[q]))
        order = order[np.isfinite(d[q][order])][:k_eff]
        if len(order) < k_eff:
            raise ValueError("non-finite features: query %d has %d of %d neighbours" % (q, len(order), k_eff))
        idx[q, :k_eff] = order
        dist[q, :k_eff] = d[q][order]
    return idx, dist


def match_knn(src_feat, dst_feat, k, mutual=True):
    """The sorted (src, dst) int32 pairs: (i, j) with j in F[i] -- with mutual also i in B[j] -- where F[i] = the k
    nearest target rows of source row i and B[j] = the k nearest source rows of target row j."""
    src, dst = np.asarray(src_feat, dtype=np.float32), np.asarray(dst_feat, dtype=np.float32)
    if src.shape[0] == 0 or dst.shape[0] == 0:
        return np.zeros((0, 2), dtype=np.int32)
    F = knn(dst, src, k)[0]
    B = knn(src, dst, k)[0] if mutual else None
    pairs = []
    for i in range(src.shape[0]):
        for j in sorted(int(j) for j in F[i] if j >= 0):
            if B is None or i in B[j]:
                pairs.append((i, j))
    return np.array(pairs, dtype=np.int32).reshape(-1, 2)
