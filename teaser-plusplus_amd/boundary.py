"""Boundary points on the GPU: ``compute_boundary_points(points, normals, radius, max_nn, angle_threshold)`` is Open3D's
``PointCloud.compute_boundary_points`` (the angle criterion of PCL's ``BoundaryEstimation``): a point is a boundary point
when the directions to its neighbours, projected onto its tangent plane, leave an angular gap above the threshold.
``boundary_mask`` returns the mask alone (with the gaps and the list lengths on request), and
``compute_boundary_points_batch`` runs many clouds in one launch sequence (every cloud's result identical to the same
cloud run alone).  FP64; the contract is written out in include/teaser_hip.h ("Boundary points"); bit parity with an
Open3D binary is not claimed.

The usual use is to drop the rim of a partial scan before descriptors are computed: normals and FPFH rows are least
reliable where the neighbourhood is half empty.

The calls run on the ICP handle of the device (one per device, shared with icp.py, calls serialised by its lock).
Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import _cloud
from .fpfh_open3d import _per_cloud, _record
from .icp import IcpNormalSearchC, _handle, _NormalSearch

_vp, _ip, _dp, _bp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)


def declare(L):
    """ctypes signature of the entry point (called by the package's lib())."""
    L.teaser_hip_icp_boundary_points_batch.argtypes = [
        _vp, C.c_int32, C.POINTER(_dp), C.POINTER(_dp), _ip, C.POINTER(IcpNormalSearchC), C.POINTER(IcpNormalSearchC), _dp,
        C.POINTER(_bp), _ip, C.POINTER(_dp), C.POINTER(_ip), C.POINTER(_dp)]


class BoundaryResult:
    """One cloud's result: ``mask`` (n bools), ``n_boundary`` (the number of True entries, counted on the device), and
    where they were asked for ``max_gap`` (n float64, radians; NaN where the normal gives no tangent frame), ``counts``
    (n int32: the length m of every point's neighbour list, the point itself included) and ``normals`` (n x 3: the
    normals the cloud was computed with)."""

    def __init__(self, mask, n_boundary, max_gap=None, counts=None, normals=None):
        self.mask, self.n_boundary, self.max_gap, self.counts, self.normals = mask, n_boundary, max_gap, counts, normals

    def select(self, points):
        """The boundary points of ``points`` (the cloud the result was computed from)."""
        return np.asarray(points)[self.mask]


def _search(search_param, radius, max_nn):
    if search_param is not None:
        return search_param
    if radius is None:
        raise ValueError("radius (with max_nn) or search_param must be given")
    return ("hybrid", float(radius), int(max_nn))


def compute_boundary_points_batch(clouds, normals, search_params, angle_threshold=90.0, normal_search=None,
                                  return_max_gap=False, return_counts=False, return_normals=False, device=-1):
    """Per cloud a BoundaryResult (include/teaser_hip.h, "Boundary points").  normals: a list with one n x 3 array per
    cloud, used as given and never normalised; an entry None (or normals=None) has the cloud's normals estimated on the
    device first, by normal_search (a KDTreeSearchParamHybrid / KDTreeSearchParamKNN, oriented or not, one for all clouds
    or a list with one per cloud) -- the bits of estimate_normals_batch followed by this call.  search_params: a
    KDTreeSearchParamHybrid / KDTreeSearchParamKNN, ("hybrid", radius, max_nn) or ("knn", k), one for all clouds or a list
    with one per cloud.  angle_threshold: degrees in [0, 360], one for all clouds or a list."""
    from . import lib
    pts = [_cloud(c, "points", kind="array of points") for c in clouds]
    b = len(pts)
    nrm = list(normals) if normals is not None else [None] * b
    if len(nrm) != b:
        raise ValueError("normals: one array (or None) per cloud")
    recs = [_record(sp, "search_param") for sp in _per_cloud(search_params, b, "search_params")]
    thr = np.array([float(t) for t in _per_cloud(angle_threshold, b, "angle_threshold")], dtype=np.float64)
    if not (np.isfinite(thr) & (thr >= 0.0) & (thr <= 360.0)).all():
        raise ValueError("angle_threshold must be finite and lie in [0, 360] degrees")
    nsp = _per_cloud(normal_search, b, "normal_search")
    nrecs = []
    for k in range(b):
        if nrm[k] is not None:
            nrm[k] = _cloud(nrm[k], "normals", kind="array of normals")
            if nrm[k].shape != pts[k].shape:
                raise ValueError("normals: cloud %d has %d points and %d normals" % (k, len(pts[k]), len(nrm[k])))
            if not np.isfinite(nrm[k]).all():
                raise ValueError("normals: cloud %d has a non-finite component" % k)
            nrecs.append(IcpNormalSearchC())
        elif isinstance(nsp[k], _NormalSearch):
            nrecs.append(nsp[k].record())
        else:
            raise ValueError("cloud %d has neither normals nor a normal_search (a KDTreeSearchParamHybrid / "
                             "KDTreeSearchParamKNN)" % k)
    mask = [np.zeros(len(p), dtype=np.uint8) for p in pts]
    gap = [np.zeros(len(p)) for p in pts] if return_max_gap else None
    cnt = [np.zeros(len(p), dtype=np.int32) for p in pts] if return_counts else None
    no = [np.zeros((len(p), 3)) for p in pts] if return_normals else None
    nb = np.zeros(b, dtype=np.int32)
    if b:
        n = np.array([len(p) for p in pts], dtype=np.int32)

        def ptrs(arrs, t=_dp):
            if arrs is None:
                return None
            return (t * b)(*[None if a is None or len(a) == 0 else a.ctypes.data_as(t) for a in arrs])
        _handle(device).call(lib().teaser_hip_icp_boundary_points_batch, b, ptrs(pts), ptrs(nrm), n.ctypes.data_as(_ip),
                             (IcpNormalSearchC * b)(*recs), (IcpNormalSearchC * b)(*nrecs), thr.ctypes.data_as(_dp),
                             ptrs(mask, _bp), nb.ctypes.data_as(_ip), ptrs(gap), ptrs(cnt, _ip), ptrs(no))
    pick = lambda arrs, k: None if arrs is None else arrs[k]  # noqa: E731
    return [BoundaryResult(mask[k].astype(bool), int(nb[k]), pick(gap, k), pick(cnt, k), pick(no, k)) for k in range(b)]


def boundary_mask(points, normals=None, radius=None, max_nn=30, angle_threshold=90.0, normal_search=None,
                  search_param=None, return_max_gap=False, return_counts=False, device=-1):
    """The boolean mask of the boundary points of one cloud; with return_max_gap / return_counts a tuple (mask[,
    max_gap][, counts]).  The search is KDTreeSearchParamHybrid(radius, max_nn) unless search_param gives another one."""
    r = compute_boundary_points_batch([points], [normals], _search(search_param, radius, max_nn), angle_threshold,
                                      normal_search, return_max_gap, return_counts, device=device)[0]
    if not return_max_gap and not return_counts:
        return r.mask
    return tuple(x for x in (r.mask, r.max_gap, r.counts) if x is not None)


def compute_boundary_points(points, normals=None, radius=None, max_nn=30, angle_threshold=90.0, normal_search=None,
                            search_param=None, device=-1):
    """Open3D's PointCloud.compute_boundary_points(radius, max_nn, angle_threshold): (boundary_points, mask).  normals
    None: they are estimated on the device first, by normal_search."""
    pts = _cloud(points, "points", kind="array of points")
    mask = boundary_mask(pts, normals, radius, max_nn, angle_threshold, normal_search, search_param, device=device)
    return pts[mask], mask


__all__ = ["BoundaryResult", "boundary_mask", "compute_boundary_points", "compute_boundary_points_batch"]
