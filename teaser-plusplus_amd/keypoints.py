"""ISS keypoint detection on the GPU with Open3D's interface: ``compute_iss_keypoints(points, salient_radius,
non_max_radius, gamma_21, gamma_32, min_neighbors)`` returns the indices of the keypoints in ascending order (Open3D's
``o3d.geometry.keypoint.compute_iss_keypoints`` returns the points themselves: ``points[ind]``).  Radii of 0 are
replaced by 6 and 4 times the cloud's resolution, as Open3D does.  ``compute_iss_keypoints_batch`` takes many clouds in
one launch sequence; every cloud's result is identical to the same cloud run alone.  The contract is written out in
include/teaser_hip.h ("ISS keypoints").

The calls run on the ICP handle of the device (one per device, shared with icp.py and outlier.py).  Without a GPU they
raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from .icp import _handle
from .outlier import _clouds, _per_cloud

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
_bp = C.POINTER(C.c_uint8)


class ISSParamsC(C.Structure):
    """teaser_icp_iss_params_c"""
    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma_21", C.c_double),
                ("gamma_32", C.c_double), ("min_neighbors", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(ISSParamsC) == 40


def declare(L):
    """ctypes signatures of the ISS entry points (called by the package's lib())."""
    L.teaser_hip_icp_iss_params_default.argtypes = [C.POINTER(ISSParamsC)]
    L.teaser_hip_icp_iss_keypoints_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(ISSParamsC),
                                                     C.POINTER(_bp), _ip, C.POINTER(_dp), C.POINTER(_ip), _dp]


def compute_iss_keypoints_batch(clouds, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975,
                                min_neighbors=5, return_saliency=False, device=-1):
    """Per cloud the int64 indices of its ISS keypoints in ascending order.  Every parameter: one value for all clouds
    or one per cloud.  return_saliency=True: per cloud (indices, details), details a dict with the per-point "saliency"
    (the smallest eigenvalue where both ratio tests pass, else 0), "count" (n x 2: neighbours inside salient_radius and
    inside non_max_radius, the point included) and the cloud's "resolution" (NaN when the radii were given),
    "salient_radius" and "non_max_radius" as used."""
    from . import lib
    pts, n, pp = _clouds(clouds)
    b = len(pts)
    cols = [_per_cloud(v, b, t, w) for v, t, w in ((salient_radius, np.float64, "salient_radius"),
                                                   (non_max_radius, np.float64, "non_max_radius"),
                                                   (gamma_21, np.float64, "gamma_21"), (gamma_32, np.float64, "gamma_32"),
                                                   (min_neighbors, np.int32, "min_neighbors"))]
    rec = (ISSParamsC * max(b, 1))()
    for c in range(b):
        rec[c] = ISSParamsC(float(cols[0][c]), float(cols[1][c]), float(cols[2][c]), float(cols[3][c]),
                            int(cols[4][c]), 0)
    keep = [np.zeros(len(p), dtype=np.uint8) for p in pts]
    sal = [np.zeros(len(p), dtype=np.float64) for p in pts]
    cnt = [np.zeros((len(p), 2), dtype=np.int32) for p in pts]
    kept = np.zeros(max(b, 1), dtype=np.int32)
    radii = np.full((max(b, 1), 3), np.nan)
    if b:
        kp = (_bp * b)(*[a.ctypes.data_as(_bp) for a in keep])
        sp = (_dp * b)(*[a.ctypes.data_as(_dp) for a in sal]) if return_saliency else None
        cp = (_ip * b)(*[a.ctypes.data_as(_ip) for a in cnt]) if return_saliency else None
        _handle(device).call(lib().teaser_hip_icp_iss_keypoints_batch, b, pp, n.ctypes.data_as(_ip), rec, kp,
                             kept.ctypes.data_as(_ip), sp, cp, radii.ctypes.data_as(_dp) if return_saliency else None)
    out = []
    for c in range(b):
        ind = np.flatnonzero(keep[c])
        assert len(ind) == kept[c]
        if return_saliency:
            out.append((ind, dict(saliency=sal[c], count=cnt[c], resolution=float(radii[c, 0]),
                                  salient_radius=float(radii[c, 1]), non_max_radius=float(radii[c, 2]))))
        else:
            out.append(ind)
    return out


def compute_iss_keypoints(points, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975,
                          min_neighbors=5, return_saliency=False, device=-1):
    """compute_iss_keypoints_batch for one n x 3 cloud."""
    return compute_iss_keypoints_batch([points], salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors,
                                       return_saliency, device)[0]
