"""Farthest-point down-sampling on the GPU with Open3D's interface: ``farthest_point_down_sample(points, num_samples,
start_index=0)`` returns the num_samples x 3 points ``pcd.farthest_point_down_sample`` selects, in the order it selects
them; ``farthest_point_indices`` returns their indices, and ``farthest_point_down_sample_batch`` takes many clouds in one
call, every cloud's result identical to the same cloud run alone.  The contract is written out in include/teaser_hip.h
("Farthest-point down-sampling").

The calls run on the ICP handle of the device (one per device, shared with icp.py, outlier.py, keypoints.py and
cluster.py); its option "fps_resident_max" (outlier.set_icp_option) moves the boundary between the two routes and changes
no result.  Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from .icp import _handle
from .outlier import _clouds, _per_cloud

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)


class FPSParamsC(C.Structure):
    """teaser_icp_fps_params_c"""
    _fields_ = [("num_samples", C.c_int32), ("start_index", C.c_int32)]


assert C.sizeof(FPSParamsC) == 8


def declare(L):
    """ctypes signature of the farthest-point entry point (called by the package's lib())."""
    L.teaser_hip_icp_farthest_point_down_sample_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip,
                                                                  C.POINTER(FPSParamsC), C.POINTER(_ip), C.POINTER(_dp),
                                                                  C.POINTER(_dp)]


def farthest_point_down_sample_batch(clouds, num_samples, start_index=0, return_sel_dist=False, return_final_dist=False,
                                     device=-1):
    """Per cloud the int32 indices of its num_samples samples in the order of selection (the first is start_index).
    num_samples and start_index: one value for all clouds or one per cloud.  return_sel_dist=True appends the per-cloud
    list of float64 arrays with the squared distance of every sample to the nearest earlier one (+inf for the first),
    return_final_dist=True the per-cloud list with the squared distance of every point to its nearest sample, in that
    order; with neither the list of index arrays is returned alone."""
    from . import lib
    pts, n, pp = _clouds(clouds)
    b = len(pts)
    ks = _per_cloud(num_samples, b, np.int64, "num_samples")
    ss = _per_cloud(start_index, b, np.int64, "start_index")
    i32 = np.iinfo(np.int32)
    if b and (min(ks.min(), ss.min()) < i32.min or max(ks.max(), ss.max()) > i32.max):
        raise ValueError("num_samples and start_index must fit 32 bits")
    rec = (FPSParamsC * max(b, 1))()
    for c in range(b):
        rec[c] = FPSParamsC(int(ks[c]), int(ss[c]))
    index = [np.zeros(max(int(k), 0), dtype=np.int32) for k in ks]
    sel = [np.zeros(max(int(k), 0), dtype=np.float64) for k in ks]
    fin = [np.zeros(len(p), dtype=np.float64) for p in pts]
    if b:
        xp = (_ip * b)(*[a.ctypes.data_as(_ip) for a in index])
        sp = (_dp * b)(*[a.ctypes.data_as(_dp) for a in sel]) if return_sel_dist else None
        fp = (_dp * b)(*[a.ctypes.data_as(_dp) for a in fin]) if return_final_dist else None
        _handle(device).call(lib().teaser_hip_icp_farthest_point_down_sample_batch, b, pp, n.ctypes.data_as(_ip), rec,
                             xp, sp, fp)
    if not (return_sel_dist or return_final_dist):
        return index
    out = (index,)
    if return_sel_dist:
        out += (sel,)
    if return_final_dist:
        out += (fin,)
    return out


def farthest_point_indices(points, num_samples, start_index=0, return_sel_dist=False, return_final_dist=False,
                           device=-1):
    """farthest_point_down_sample_batch for one n x 3 cloud: the int32 indices (with return_sel_dist /
    return_final_dist: a tuple of the indices and the arrays asked for, in that order).  The loop runs as stated also
    for num_samples == n."""
    out = farthest_point_down_sample_batch([points], num_samples, start_index, return_sel_dist, return_final_dist,
                                           device)
    if not (return_sel_dist or return_final_dist):
        return out[0]
    return tuple(x[0] for x in out)


def farthest_point_down_sample(points, num_samples, start_index=0, device=-1):
    """Open3D's pcd.farthest_point_down_sample(num_samples, start_index) on an n x 3 array: the num_samples x 3 points
    in the order of selection.  num_samples == n returns the cloud itself in input order (Open3D's shortcut)."""
    pts = _clouds([points])[0][0]
    if num_samples == len(pts):
        return pts.copy()
    return pts[farthest_point_indices(pts, num_samples, start_index, device=device)]
