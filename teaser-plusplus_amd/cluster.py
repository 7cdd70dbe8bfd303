"""DBSCAN clustering on the GPU with Open3D's interface: ``cluster_dbscan(points, eps, min_points)`` returns one int32
label per point, ``-1`` for noise, clusters numbered from 0 in the order Open3D's loop opens them (ascending smallest
core index).  ``cluster_dbscan_batch`` takes many clouds in one launch sequence; every cloud's result is identical to
the same cloud run alone.  The contract is written out in include/teaser_hip.h ("DBSCAN clustering").

The calls run on the ICP handle of the device (one per device, shared with icp.py, outlier.py and keypoints.py).
Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from .icp import _handle
from .outlier import _clouds, _per_cloud

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)


class DBSCANParamsC(C.Structure):
    """teaser_icp_dbscan_params_c"""
    _fields_ = [("eps", C.c_double), ("min_points", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(DBSCANParamsC) == 16


def declare(L):
    """ctypes signature of the DBSCAN entry point (called by the package's lib())."""
    L.teaser_hip_icp_cluster_dbscan_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(DBSCANParamsC),
                                                      C.POINTER(_ip), _ip, C.POINTER(_ip), C.POINTER(_ip)]


def cluster_dbscan_batch(clouds, eps, min_points, return_counts=False, return_roots=False, device=-1):
    """(labels, n_clusters): per cloud its int32 labels, and an int32 array with the number of clusters of each cloud.
    eps and min_points: one value for all clouds or one per cloud.  return_counts=True appends the per-cloud list of
    neighbour counts (the point itself included), return_roots=True the per-cloud list of roots (the smallest core
    index of a core point's component, -1 for a point that is not core), in that order."""
    from . import lib
    pts, n, pp = _clouds(clouds)
    b = len(pts)
    e = _per_cloud(eps, b, np.float64, "eps")
    m = _per_cloud(min_points, b, np.int32, "min_points")
    rec = (DBSCANParamsC * max(b, 1))()
    for c in range(b):
        rec[c] = DBSCANParamsC(float(e[c]), int(m[c]), 0)
    labels = [np.full(len(p), -1, dtype=np.int32) for p in pts]
    counts = [np.zeros(len(p), dtype=np.int32) for p in pts]
    roots = [np.full(len(p), -1, dtype=np.int32) for p in pts]
    ncl = np.zeros(b, dtype=np.int32)
    if b:
        lp = (_ip * b)(*[a.ctypes.data_as(_ip) for a in labels])
        cp = (_ip * b)(*[a.ctypes.data_as(_ip) for a in counts]) if return_counts else None
        rp = (_ip * b)(*[a.ctypes.data_as(_ip) for a in roots]) if return_roots else None
        _handle(device).call(lib().teaser_hip_icp_cluster_dbscan_batch, b, pp, n.ctypes.data_as(_ip), rec, lp,
                             ncl.ctypes.data_as(_ip), cp, rp)
    out = (labels, ncl)
    if return_counts:
        out += (counts,)
    if return_roots:
        out += (roots,)
    return out


def cluster_dbscan(points, eps, min_points, return_counts=False, return_roots=False, device=-1):
    """cluster_dbscan_batch for one n x 3 cloud: the int32 labels (with return_counts / return_roots: a tuple of the
    labels and the arrays asked for, in that order)."""
    out = cluster_dbscan_batch([points], eps, min_points, return_counts, return_roots, device)
    extra = tuple(x[0] for x in out[2:])
    return (out[0][0],) + extra if extra else out[0][0]
