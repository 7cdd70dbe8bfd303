"""Point-cloud cleaning on the GPU with Open3D's interface: ``remove_statistical_outlier(points, nb_neighbors,
std_ratio)`` and ``remove_radius_outlier(points, nb_points, radius)`` return ``(points[ind], ind)`` like
``pcd.remove_statistical_outlier`` / ``pcd.remove_radius_outlier``; ``self_knn(points, k)`` is the neighbour search the
statistical rule is built on (the k nearest points of the same cloud, the point itself included, no radius).  Each has a
``_batch`` form: many clouds, one launch sequence, every cloud's result identical to the same cloud run alone.  The
contracts are written out in include/teaser_hip.h ("Self k-NN", "Outlier removal").

The calls run on the ICP handle of the device (one per device, shared with icp.py, calls serialised by its lock).
Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import _cloud
from .icp import _handle

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
_bp = C.POINTER(C.c_uint8)

KNN_MAX = 100  # TEASER_HIP_ICP_KNN_MAX


def declare(L):
    """ctypes signatures of the self k-NN / outlier-removal entry points (called by the package's lib())."""
    L.teaser_hip_icp_self_knn_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, _ip, C.POINTER(_ip),
                                                C.POINTER(_dp)]
    L.teaser_hip_icp_remove_statistical_outliers_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, _ip, _dp,
                                                                   C.POINTER(_bp), _ip, C.POINTER(_dp), _dp]
    L.teaser_hip_icp_remove_radius_outliers_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, _ip, _dp,
                                                              C.POINTER(_bp), _ip, C.POINTER(_ip)]
    L.teaser_hip_icp_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
    L.teaser_hip_icp_get_option.argtypes = [_vp, C.c_char_p, C.POINTER(C.c_int64)]


def _clouds(clouds):
    pts = [_cloud(c, "points", kind="array of points") for c in clouds]
    n = np.array([len(p) for p in pts], dtype=np.int32)
    pp = (_dp * max(len(pts), 1))(*[p.ctypes.data_as(_dp) for p in pts])
    return pts, n, pp


def _per_cloud(v, b, dtype, what):
    a = np.asarray(v)
    if a.ndim > 1 or (a.ndim == 1 and len(a) != b):
        raise ValueError("%s: one value for all clouds or one per cloud" % what)
    return np.ascontiguousarray(np.broadcast_to(a, (b,)).astype(dtype))


def set_icp_option(name, value, device=-1):
    """teaser_hip_icp_set_option on the device's ICP handle ("knn_ring_cap": 0 .. 16, default 4; "fps_resident_max":
    0 .. 10240, the default; see fps.py; "fpfh_list_bytes": 1 .. 2^40, default 512 MiB; see fpfh_open3d.py).  The handle is the
    one every call of this module and of icp.py shares for that device, so the setting is global to the device and
    stays until it is set again; it changes the cost of a search, never a result."""
    from . import lib
    _handle(device).call(lib().teaser_hip_icp_set_option, name.encode(), int(value))


def get_icp_option(name, device=-1):
    """teaser_hip_icp_get_option on the device's ICP handle ("knn_ring_cap", "knn_fallbacks", "fps_resident_max",
    "fpfh_list_bytes")."""
    from . import lib
    v = C.c_int64(0)
    _handle(device).call(lib().teaser_hip_icp_get_option, name.encode(), C.byref(v))
    return int(v.value)


def self_knn_batch(clouds, k, return_distance=False, device=-1):
    """Per cloud an n x k int32 array: row i holds the min(k, n) nearest points of the same cloud in ascending
    (squared distance, index), i itself included, then -1.  k: one value for all clouds or one per cloud, in [1, 100].
    return_distance=True: a list of (indices, squared distances) with +inf in the unused slots."""
    from . import lib
    pts, n, pp = _clouds(clouds)
    b = len(pts)
    ks = _per_cloud(k, b, np.int32, "k")
    if b and (ks.min() < 1 or ks.max() > KNN_MAX):
        raise ValueError("k must lie in [1, %d]" % KNN_MAX)
    idx = [np.empty((len(p), int(kk)), dtype=np.int32) for p, kk in zip(pts, ks)]
    d2 = [np.empty((len(p), int(kk)), dtype=np.float64) for p, kk in zip(pts, ks)] if return_distance else None
    if b:
        ip = (_ip * b)(*[a.ctypes.data_as(_ip) for a in idx])
        dp = (_dp * b)(*[a.ctypes.data_as(_dp) for a in d2]) if return_distance else None
        _handle(device).call(lib().teaser_hip_icp_self_knn_batch, b, pp, n.ctypes.data_as(_ip),
                             ks.ctypes.data_as(_ip), ip, dp)
    return list(zip(idx, d2)) if return_distance else idx


def self_knn(points, k, return_distance=False, device=-1):
    """self_knn_batch for one cloud."""
    return self_knn_batch([points], k, return_distance, device)[0]


def remove_statistical_outlier_batch(clouds, nb_neighbors, std_ratio, return_stats=False, device=-1):
    """Open3D's remove_statistical_outlier for many clouds in one launch sequence.  nb_neighbors (in [1, 100]) and
    std_ratio (> 0): one value for all clouds or one per cloud.  Returns per cloud (points[ind], ind), ind the kept
    indices in ascending order; with return_stats=True (points[ind], ind, stats), stats a dict with the per-point
    mean neighbour distance "avg" and the cloud's "mean", "std" and "threshold"."""
    from . import lib
    pts, n, pp = _clouds(clouds)
    b = len(pts)
    ks = _per_cloud(nb_neighbors, b, np.int32, "nb_neighbors")
    rs = _per_cloud(std_ratio, b, np.float64, "std_ratio")
    if b and (ks.min() < 1 or ks.max() > KNN_MAX):
        raise ValueError("nb_neighbors must lie in [1, %d]" % KNN_MAX)
    if b and not (np.isfinite(rs).all() and (rs > 0).all()):
        raise ValueError("std_ratio must be finite and > 0")
    keep = [np.zeros(len(p), dtype=np.uint8) for p in pts]
    avg = [np.empty(len(p), dtype=np.float64) for p in pts]
    kept = np.zeros(max(b, 1), dtype=np.int32)
    stats = np.full((max(b, 1), 3), np.nan)
    if b:
        kp = (_bp * b)(*[a.ctypes.data_as(_bp) for a in keep])
        ap = (_dp * b)(*[a.ctypes.data_as(_dp) for a in avg]) if return_stats else None
        _handle(device).call(lib().teaser_hip_icp_remove_statistical_outliers_batch, b, pp, n.ctypes.data_as(_ip),
                             ks.ctypes.data_as(_ip), rs.ctypes.data_as(_dp), kp, kept.ctypes.data_as(_ip), ap,
                             stats.ctypes.data_as(_dp) if return_stats else None)
    out = []
    for c in range(b):
        ind = np.flatnonzero(keep[c])
        assert len(ind) == kept[c]
        if return_stats:
            out.append((pts[c][ind], ind, dict(avg=avg[c], mean=float(stats[c, 0]), std=float(stats[c, 1]),
                                               threshold=float(stats[c, 2]))))
        else:
            out.append((pts[c][ind], ind))
    return out


def remove_statistical_outlier(points, nb_neighbors, std_ratio, return_stats=False, device=-1):
    """Open3D's pcd.remove_statistical_outlier(nb_neighbors, std_ratio) on an n x 3 array: (points[ind], ind)."""
    return remove_statistical_outlier_batch([points], nb_neighbors, std_ratio, return_stats, device)[0]


def remove_radius_outlier_batch(clouds, nb_points, radius, return_counts=False, device=-1):
    """Open3D's remove_radius_outlier for many clouds in one launch sequence: a point is kept iff more than nb_points
    points of its cloud (itself included) lie closer than radius.  nb_points (>= 1) and radius (> 0): one value for all
    clouds or one per cloud.  Returns per cloud (points[ind], ind), with return_counts=True (points[ind], ind, counts)."""
    from . import lib
    pts, n, pp = _clouds(clouds)
    b = len(pts)
    ks = _per_cloud(nb_points, b, np.int32, "nb_points")
    rs = _per_cloud(radius, b, np.float64, "radius")
    if b and ks.min() < 1:
        raise ValueError("nb_points must be >= 1")
    if b and not (np.isfinite(rs).all() and (rs > 0).all()):
        raise ValueError("radius must be finite and > 0")
    keep = [np.zeros(len(p), dtype=np.uint8) for p in pts]
    cnt = [np.empty(len(p), dtype=np.int32) for p in pts]
    kept = np.zeros(max(b, 1), dtype=np.int32)
    if b:
        kp = (_bp * b)(*[a.ctypes.data_as(_bp) for a in keep])
        cp = (_ip * b)(*[a.ctypes.data_as(_ip) for a in cnt]) if return_counts else None
        _handle(device).call(lib().teaser_hip_icp_remove_radius_outliers_batch, b, pp, n.ctypes.data_as(_ip),
                             ks.ctypes.data_as(_ip), rs.ctypes.data_as(_dp), kp, kept.ctypes.data_as(_ip), cp)
    out = []
    for c in range(b):
        ind = np.flatnonzero(keep[c])
        assert len(ind) == kept[c]
        out.append((pts[c][ind], ind, cnt[c]) if return_counts else (pts[c][ind], ind))
    return out


def remove_radius_outlier(points, nb_points, radius, return_counts=False, device=-1):
    """Open3D's pcd.remove_radius_outlier(nb_points, radius) on an n x 3 array: (points[ind], ind)."""
    return remove_radius_outlier_batch([points], nb_points, radius, return_counts, device)[0]
