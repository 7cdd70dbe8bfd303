"""Nearest-neighbour search between two clouds on the GPU with Open3D's interface: the k nearest, the neighbours inside a
radius (uncapped, variable length) and the hybrid of both, for a query set that is not the data cloud.
``knn_search(data, queries, k)``, ``hybrid_search(data, queries, radius, max_nn)`` and
``radius_search(data, queries, radius)`` are the plain calls, each with a ``_batch`` form (many problems, one launch
sequence, every problem's result identical to the same problem run alone); ``NearestNeighborSearch(points)`` has the
method names of ``open3d.core.nns.NearestNeighborSearch``, ``KDTreeFlann(points)`` those of
``open3d.geometry.KDTreeFlann``; ``compute_point_cloud_distance`` and ``compute_nearest_neighbor_distance`` are the
point-cloud methods of the same names.  Distances are squared, neighbours come in ascending (squared distance, index);
the contract is written out in include/teaser_hip.h ("Neighbour search").

The calls run on the ICP handle of the device (one per device, shared with icp.py, calls serialised by its lock).
Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import _cloud
from .icp import _handle
from .outlier import KNN_MAX, _per_cloud, self_knn

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
_lp = C.POINTER(C.c_int64)


def declare(L):
    """ctypes signatures of the neighbour-search entry points (called by the package's lib())."""
    L.teaser_hip_icp_knn_search_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, _ip,
                                                  C.POINTER(_ip), C.POINTER(_dp)]
    L.teaser_hip_icp_hybrid_search_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, _dp, _ip,
                                                     C.POINTER(_ip), C.POINTER(_dp), C.POINTER(_ip)]
    L.teaser_hip_icp_radius_search_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, _dp, _lp,
                                                     C.POINTER(_ip), C.POINTER(_ip), C.POINTER(_dp), _lp]


def _side(clouds, what):
    pts = [_cloud(c, what, kind="array of points") for c in clouds]
    n = np.array([len(p) for p in pts], dtype=np.int32)
    pp = (_dp * max(len(pts), 1))(*[p.ctypes.data_as(_dp) for p in pts])
    return pts, n, pp


def _pairs(data, queries):
    if len(data) != len(queries):
        raise ValueError("as many query sets as data clouds")
    return _side(data, "data"), _side(queries, "queries")


def _pointers(arrays, ptr):
    return (ptr * max(len(arrays), 1))(*[a.ctypes.data_as(ptr) for a in arrays])


def _radii(radius, b):
    rs = _per_cloud(radius, b, np.float64, "radius")
    if b and not (np.isfinite(rs).all() and (rs > 0).all()):
        raise ValueError("radius must be finite and > 0")
    return rs


def _counts(k, b, what):
    ks = _per_cloud(k, b, np.int32, what)
    if b and (ks.min() < 1 or ks.max() > KNN_MAX):
        raise ValueError("%s must lie in [1, %d]" % (what, KNN_MAX))
    return ks


def knn_search_batch(data, queries, k, device=-1):
    """Per problem (indices n_query x k int32, squared distances n_query x k float64): row i holds the min(k, n_data)
    points of data nearest to queries[i] in ascending (squared distance, index), then -1 / +inf.  k: one value for all
    problems or one per problem, in [1, 100]."""
    from . import lib
    (dat, nd, dpp), (qry, nq, qpp) = _pairs(data, queries)
    b = len(dat)
    ks = _counts(k, b, "k")
    idx = [np.empty((len(q), int(kk)), dtype=np.int32) for q, kk in zip(qry, ks)]
    d2 = [np.empty((len(q), int(kk)), dtype=np.float64) for q, kk in zip(qry, ks)]
    if b:
        _handle(device).call(lib().teaser_hip_icp_knn_search_batch, b, dpp, nd.ctypes.data_as(_ip), qpp,
                             nq.ctypes.data_as(_ip), ks.ctypes.data_as(_ip), _pointers(idx, _ip), _pointers(d2, _dp))
    return list(zip(idx, d2))


def knn_search(data, queries, k, device=-1):
    """knn_search_batch for one problem: (indices, squared distances)."""
    return knn_search_batch([data], [queries], k, device)[0]


def hybrid_search_batch(data, queries, radius, max_nn, device=-1):
    """Per problem (indices n_query x max_nn int32, squared distances, counts n_query int32): row i holds the first
    min(max_nn, number inside) points of data with squared distance < radius^2 (strict) in ascending (squared distance,
    index), then -1 / +inf; counts[i] is the number written.  radius (> 0) and max_nn (in [1, 100]): one value for all
    problems or one per problem."""
    from . import lib
    (dat, nd, dpp), (qry, nq, qpp) = _pairs(data, queries)
    b = len(dat)
    rs = _radii(radius, b)
    ks = _counts(max_nn, b, "max_nn")
    idx = [np.empty((len(q), int(kk)), dtype=np.int32) for q, kk in zip(qry, ks)]
    d2 = [np.empty((len(q), int(kk)), dtype=np.float64) for q, kk in zip(qry, ks)]
    cnt = [np.empty(len(q), dtype=np.int32) for q in qry]
    if b:
        _handle(device).call(lib().teaser_hip_icp_hybrid_search_batch, b, dpp, nd.ctypes.data_as(_ip), qpp,
                             nq.ctypes.data_as(_ip), rs.ctypes.data_as(_dp), ks.ctypes.data_as(_ip),
                             _pointers(idx, _ip), _pointers(d2, _dp), _pointers(cnt, _ip))
    return list(zip(idx, d2, cnt))


def hybrid_search(data, queries, radius, max_nn, device=-1):
    """hybrid_search_batch for one problem: (indices, squared distances, counts)."""
    return hybrid_search_batch([data], [queries], radius, max_nn, device)[0]


def radius_search_batch(data, queries, radius, max_total=None, device=-1):
    """Per problem (indices int32, squared distances float64, row_splits int64 of length n_query + 1): the neighbours of
    queries[i] -- every point of data with squared distance < radius^2 (strict), in ascending (squared distance, index)
    -- are indices[row_splits[i]:row_splits[i + 1]].  Without max_total the call counts first and fills arrays of the
    exact size in a second call; max_total (one value for all problems or one per problem: a guess of a problem's number
    of entries) allows a single call when every guess suffices, and costs the second call only where one does not."""
    from . import lib
    (dat, nd, dpp), (qry, nq, qpp) = _pairs(data, queries)
    b = len(dat)
    rs = _radii(radius, b)
    if b == 0:
        return []
    cnt = [np.zeros(len(q), dtype=np.int32) for q in qry]
    total = np.zeros(b, dtype=np.int64)
    call = lib().teaser_hip_icp_radius_search_batch
    head = (b, dpp, nd.ctypes.data_as(_ip), qpp, nq.ctypes.data_as(_ip), rs.ctypes.data_as(_dp))
    cap = np.zeros(b, dtype=np.int64)
    idx = d2 = None
    if max_total is not None:
        cap = _per_cloud(max_total, b, np.int64, "max_total")
        if cap.min() < 0:
            raise ValueError("max_total must be >= 0")
        idx = [np.empty(int(c), dtype=np.int32) for c in cap]
        d2 = [np.empty(int(c), dtype=np.float64) for c in cap]
        _handle(device).call(call, *head, cap.ctypes.data_as(_lp), _pointers(cnt, _ip), _pointers(idx, _ip),
                             _pointers(d2, _dp), total.ctypes.data_as(_lp))
    else:
        _handle(device).call(call, *head, None, _pointers(cnt, _ip), None, None, total.ctypes.data_as(_lp))
    if idx is None or (total > cap).any():  # the fill half, at the exact sizes
        cap = total.copy()
        idx = [np.empty(int(c), dtype=np.int32) for c in cap]
        d2 = [np.empty(int(c), dtype=np.float64) for c in cap]
        _handle(device).call(call, *head, cap.ctypes.data_as(_lp), _pointers(cnt, _ip), _pointers(idx, _ip),
                             _pointers(d2, _dp), total.ctypes.data_as(_lp))
    out = []
    for c in range(b):
        splits = np.zeros(len(cnt[c]) + 1, dtype=np.int64)
        np.cumsum(cnt[c], out=splits[1:])
        assert splits[-1] == total[c]
        out.append((idx[c][:total[c]], d2[c][:total[c]], splits))
    return out


def radius_search(data, queries, radius, max_total=None, device=-1):
    """radius_search_batch for one problem: (indices, squared distances, row_splits)."""
    return radius_search_batch([data], [queries], radius, max_total, device)[0]


class NearestNeighborSearch:
    """open3d.core.nns.NearestNeighborSearch on an n x 3 array of data points.  There is no index to build in advance
    (Open3D's knn_index() and its siblings have no counterpart): the hash grid depends on k or on the radius and is built
    by every search."""

    def __init__(self, points, device=-1):
        self.points = _cloud(points, "points", kind="array of points")
        self.device = device

    def knn_search(self, query_points, knn):
        """(indices, squared distances), each n_query x knn."""
        return knn_search(self.points, query_points, knn, self.device)

    def fixed_radius_search(self, query_points, radius, max_total=None):
        """(indices, squared distances, row_splits)."""
        return radius_search(self.points, query_points, radius, max_total, self.device)

    def hybrid_search(self, query_points, radius, max_knn):
        """(indices, squared distances, counts)."""
        return hybrid_search(self.points, query_points, radius, max_knn, self.device)


class KDTreeFlann:
    """open3d.geometry.KDTreeFlann on an n x 3 array of data points: one query per call, (count, indices, squared
    distances) like Open3D's search_*_vector_3d."""

    def __init__(self, points, device=-1):
        self.points = _cloud(points, "points", kind="array of points")
        self.device = device

    def _query(self, query):
        return np.asarray(query, dtype=np.float64).reshape(1, 3)

    def search_knn_vector_3d(self, query, knn):
        idx, d2 = knn_search(self.points, self._query(query), knn, self.device)
        m = int((idx[0] >= 0).sum())
        return m, idx[0, :m].copy(), d2[0, :m].copy()

    def search_radius_vector_3d(self, query, radius):
        idx, d2, _ = radius_search(self.points, self._query(query), radius, None, self.device)
        return len(idx), idx, d2

    def search_hybrid_vector_3d(self, query, radius, max_nn):
        idx, d2, cnt = hybrid_search(self.points, self._query(query), radius, max_nn, self.device)
        m = int(cnt[0])
        return m, idx[0, :m].copy(), d2[0, :m].copy()


def compute_point_cloud_distance(source, target, device=-1):
    """Open3D's source.compute_point_cloud_distance(target): per source point the distance to the nearest target point
    (the square root of the k = 1 squared distance; +inf when target is empty)."""
    _, d2 = knn_search(target, source, 1, device)
    return np.sqrt(d2[:, 0])


def compute_nearest_neighbor_distance(points, device=-1):
    """Open3D's pcd.compute_nearest_neighbor_distance(): per point the distance to its nearest other point (the square
    root of slot 1 of self k-NN with k = 2); zeros for fewer than two points."""
    pts = _cloud(points, "points", kind="array of points")
    if len(pts) < 2:
        return np.zeros(len(pts))
    _, d2 = self_knn(pts, 2, return_distance=True, device=device)
    return np.sqrt(d2[:, 1])
