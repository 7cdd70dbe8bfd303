"""FPFH in Open3D's form on the GPU: ``compute_fpfh_feature(points, normals, search_param)`` is
``open3d.pipelines.registration.compute_fpfh_feature`` on given normals with ``KDTreeSearchParamHybrid`` or
``KDTreeSearchParamKNN`` (FP64, n x 33 rows: the transpose of Open3D's 33 x n ``Feature.data``),
``compute_fpfh_feature_batch`` many clouds in one launch sequence (every cloud's result identical to the same cloud run
alone), and ``extract_fpfh(points, voxel_size)`` the two calls of the usual global-registration script: normals with
``KDTreeSearchParamHybrid(2 v, 30)``, features with ``KDTreeSearchParamHybrid(5 v, 100)``, in one call on the device.  The
contract is written out in include/teaser_hip.h ("FPFH (Open3D form)"); bit parity with an Open3D binary is not
claimed.  This is NOT the descriptor of ``compute_fpfh_batch`` / ``FPFHEstimation`` (features.py), which is PCL's.

The rows feed ``match_features``, ``registration_ransac_based_on_feature_matching`` and
``registration_fgr_based_on_feature_matching`` like those of ``compute_fpfh_batch``.

The calls run on the ICP handle of the device (one per device, shared with icp.py, calls serialised by its lock).
Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import _cloud
from .icp import IcpNormalSearchC, KDTreeSearchParamHybrid, _handle, _NormalSearch

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)

FPFH_DIM = 33
MAX_NN_RANGE = (2, 100)


class KDTreeSearchParamRadius:
    """Open3D's KDTreeSearchParamRadius(radius): a radius without a cap.  It exists to be refused by name: the descriptor
    (like the normals) is an ordered sum over a bounded sorted list, and without a cap there is no such list."""

    def __init__(self, radius):
        self.radius = float(radius)

    def __repr__(self):
        return "KDTreeSearchParamRadius(radius=%g)" % self.radius


def declare(L):
    """ctypes signature of the entry point (called by the package's lib())."""
    L.teaser_hip_icp_fpfh_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), C.POINTER(_dp), _ip,
                                            C.POINTER(IcpNormalSearchC), C.POINTER(IcpNormalSearchC), C.POINTER(_dp),
                                            C.POINTER(_dp), C.POINTER(_dp)]


def _record(sp, what):
    """The search record of the descriptor.  Besides the two classes, ("hybrid", radius, max_nn) and ("knn", k) are
    accepted: the classes refuse max_nn = 2, which the descriptor allows."""
    if isinstance(sp, KDTreeSearchParamRadius):
        raise ValueError("%s: KDTreeSearchParamRadius is not supported (it is uncapped: there is no bounded sorted list "
                         "to sum over); use KDTreeSearchParamHybrid or KDTreeSearchParamKNN" % what)
    if isinstance(sp, _NormalSearch):
        if sp.orient != 0:
            raise ValueError("%s: an oriented search parameter (orient != 0) has no meaning here" % what)
        search, radius, max_nn = sp.search, sp.radius, sp.max_nn
    elif isinstance(sp, tuple) and len(sp) == 3 and sp[0] == "hybrid":
        search, radius, max_nn = 0, float(sp[1]), int(sp[2])
    elif isinstance(sp, tuple) and len(sp) == 2 and sp[0] == "knn":
        search, radius, max_nn = 1, 0.0, int(sp[1])
    else:
        raise ValueError("%s: a KDTreeSearchParamHybrid / KDTreeSearchParamKNN, (\"hybrid\", radius, max_nn) or "
                         "(\"knn\", k)" % what)
    if not MAX_NN_RANGE[0] <= max_nn <= MAX_NN_RANGE[1]:
        raise ValueError("%s: max_nn / knn must lie in [%d, %d]" % ((what,) + MAX_NN_RANGE))
    if search == 0 and not (np.isfinite(radius) and radius > 0):
        raise ValueError("%s: radius must be finite and > 0" % what)
    return IcpNormalSearchC(search, max_nn, radius, 0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))


def _per_cloud(v, b, what):
    vs = list(v) if isinstance(v, list) else [v] * b
    if len(vs) != b:
        raise ValueError("%s: one for all clouds or a list with one per cloud" % what)
    return vs


def compute_fpfh_feature_batch(clouds, normals, search_params, normal_search=None, return_spfh=False,
                               return_normals=False, device=-1):
    """Per cloud the n x 33 float64 FPFH rows (include/teaser_hip.h, "FPFH (Open3D form)").  normals: a list with one
    n x 3 array of unit normals per cloud, used as given; an entry None (or normals=None) has the cloud's normals
    estimated on the device first, by normal_search (a KDTreeSearchParamHybrid / KDTreeSearchParamKNN, oriented or not,
    one for all clouds or a list with one per cloud) -- the bits of estimate_normals_batch followed by this call.
    search_params: one for all clouds or a list with one per cloud.  With return_spfh / return_normals each entry is a
    tuple (fpfh[, spfh n x 33][, normals n x 3])."""
    from . import lib
    pts = [_cloud(c, "points", kind="array of points") for c in clouds]
    b = len(pts)
    nrm = list(normals) if normals is not None else [None] * b
    if len(nrm) != b:
        raise ValueError("normals: one array (or None) per cloud")
    recs = [_record(sp, "search_param") for sp in _per_cloud(search_params, b, "search_params")]
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
    fp = [np.zeros((len(p), FPFH_DIM)) for p in pts]
    sp = [np.zeros((len(p), FPFH_DIM)) for p in pts] if return_spfh else None
    no = [np.zeros((len(p), 3)) for p in pts] if return_normals else None
    if b:
        n = np.array([len(p) for p in pts], dtype=np.int32)
        ptrs = lambda arrs: None if arrs is None else (_dp * b)(  # noqa: E731
            *[None if a is None or len(a) == 0 else a.ctypes.data_as(_dp) for a in arrs])
        _handle(device).call(lib().teaser_hip_icp_fpfh_batch, b, ptrs(pts), ptrs(nrm), n.ctypes.data_as(_ip),
                             (IcpNormalSearchC * b)(*recs), (IcpNormalSearchC * b)(*nrecs), ptrs(fp), ptrs(sp), ptrs(no))
    if not return_spfh and not return_normals:
        return fp
    return [tuple(x[k] for x in (fp, sp, no) if x is not None) for k in range(b)]


def compute_fpfh_feature(points, normals, search_param, device=-1):
    """compute_fpfh_feature_batch for one cloud with given normals: n x 33 float64."""
    if normals is None:
        raise ValueError("normals must be given (extract_fpfh and compute_fpfh_feature_batch estimate them)")
    return compute_fpfh_feature_batch([points], [normals], search_param, device=device)[0]


def extract_fpfh(points, voxel_size, return_normals=False, device=-1):
    """The extract_fpfh helper of Open3D's global-registration scripts on a (down-sampled) cloud, in one call:
    estimate_normals(KDTreeSearchParamHybrid(2 voxel_size, 30)), then compute_fpfh_feature(KDTreeSearchParamHybrid(5
    voxel_size, 100)).  Returns the n x 33 rows (with return_normals: (rows, normals))."""
    v = float(voxel_size)
    return compute_fpfh_feature_batch([points], None, KDTreeSearchParamHybrid(5 * v, 100),
                                      normal_search=KDTreeSearchParamHybrid(2 * v, 30), return_normals=return_normals,
                                      device=device)[0]


__all__ = ["KDTreeSearchParamRadius", "compute_fpfh_feature", "compute_fpfh_feature_batch", "extract_fpfh"]
