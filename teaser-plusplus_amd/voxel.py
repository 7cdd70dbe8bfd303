"""Voxel down-sampling on the GPU with Open3D's arithmetic (``pcd.voxel_down_sample(voxel_size)``):
``voxel_down_sample(points, voxel_size)`` and the batched ``voxel_down_sample_batch``.  The contract is written out in
include/teaser_hip.h ("Voxel down-sampling"): voxel index floor((p - (min_bound - v/2)) / v), output = FP64 mean of
the voxel's points summed in input order, voxels in ascending (i_x, i_y, i_z) order (Open3D's order is its hash
map's).

One library handle is kept per device between calls; calls from several threads are safe -- each handle has a lock,
so calls for one device run one after the other.  device=-1 means the calling thread's current HIP device at the
time of the call.  Without a GPU the calls raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import atexit
import ctypes as C
import threading

import numpy as np

from .icp import _current_device

_vp, _ip, _dp, _i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)


def declare(L):
    """ctypes signatures of the voxel entry points (called by the package's lib())."""
    L.teaser_hip_voxel_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_voxel_destroy.argtypes = [_vp]
    L.teaser_hip_voxel_last_error.argtypes = [_vp]
    L.teaser_hip_voxel_last_error.restype = C.c_char_p
    L.teaser_hip_voxel_down_sample_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, _dp, C.POINTER(_dp),
                                                     _i64p, C.POINTER(_ip), C.POINTER(_ip)]
    L.teaser_hip_voxel_down_sample.argtypes = [_vp, _dp, C.c_int32, C.c_double, _dp, _i64p, _ip, _ip]


# One C handle per device, shared by every thread of the process (see icp.py: a handle serves one call at a time).
_handles = {}            # device ordinal -> (handle, lock)
_handles_lock = threading.Lock()


def _handle(device):
    """(handle, lock) for `device`; device < 0 is resolved to the calling thread's current device first."""
    from . import TeaserHipError, lib
    device = int(device)
    L = lib()
    if device < 0:
        device = _current_device()
    with _handles_lock:
        entry = _handles.get(device)
        if entry is not None:
            return entry
        h = _vp()
        rc = L.teaser_hip_voxel_create(device, C.byref(h))
        if rc != 0:
            raise TeaserHipError(rc, "(no MI355X visible: the product has no CPU path)" if rc == 3 else "")
        entry = (h, threading.Lock())
        _handles[device] = entry
        return entry


@atexit.register
def _release():
    with _handles_lock:
        if not _handles:
            return
        from . import lib
        L = lib()
        for h, lock in _handles.values():
            with lock:
                L.teaser_hip_voxel_destroy(h)
        _handles.clear()


def _cloud(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.size == 0:
        return np.zeros((0, 3))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("points must be an n x 3 array, got shape %s" % (a.shape,))
    return a


def voxel_down_sample_batch(clouds, voxel_sizes, return_counts=False, return_trace=False, device=-1):
    """Down-samples many clouds (mixed sizes allowed) in one launch sequence.  voxel_sizes: one value for all clouds
    or one per cloud.  Returns a list with, per cloud, the n_out x 3 float64 voxel means -- or a tuple
    (means, counts, trace) with the parts asked for: counts[k] = points in voxel k, trace[i] = voxel of input point i.
    Each result is bit-identical to the same cloud down-sampled alone."""
    from . import TeaserHipError, lib
    pts = [_cloud(c) for c in clouds]
    b = len(pts)
    vs = np.ascontiguousarray(np.broadcast_to(np.asarray(voxel_sizes, dtype=np.float64), (b,)))
    n = np.array([len(p) for p in pts], dtype=np.int32)
    outs = [np.empty((max(int(k), 1), 3)) for k in n]
    counts = [np.empty(max(int(k), 1), dtype=np.int32) for k in n] if return_counts else None
    trace = [np.empty(max(int(k), 1), dtype=np.int32) for k in n] if return_trace else None
    n_out = np.zeros(max(b, 1), dtype=np.int64)
    h, lock = _handle(device)
    L = lib()
    pp = (_dp * max(b, 1))(*[p.ctypes.data_as(_dp) for p in pts])
    op = (_dp * max(b, 1))(*[o.ctypes.data_as(_dp) for o in outs])
    cp = None if counts is None else (_ip * max(b, 1))(*[c.ctypes.data_as(_ip) for c in counts])
    tp = None if trace is None else (_ip * max(b, 1))(*[t.ctypes.data_as(_ip) for t in trace])
    with lock:  # the handle serves one call at a time
        rc = L.teaser_hip_voxel_down_sample_batch(h, b, pp, n.ctypes.data_as(_ip), vs.ctypes.data_as(_dp), op,
                                                  n_out.ctypes.data_as(_i64p), cp, tp)
        err = L.teaser_hip_voxel_last_error(h).decode() if rc != 0 else ""
    if rc != 0:
        raise TeaserHipError(rc, err)
    res = []
    for k in range(b):
        m = int(n_out[k])
        parts = [outs[k][:m].copy()]
        if return_counts:
            parts.append(counts[k][:m].copy())
        if return_trace:
            parts.append(trace[k][:n[k]].copy())
        res.append(parts[0] if len(parts) == 1 else tuple(parts))
    return res


def voxel_down_sample(points, voxel_size, return_counts=False, return_trace=False, device=-1):
    """Open3D's pcd.voxel_down_sample(voxel_size) on an n x 3 array (np.asarray(pcd.points)): the n_out x 3 float64
    voxel means in ascending (i_x, i_y, i_z) order, or (means, counts, trace) as voxel_down_sample_batch returns."""
    return voxel_down_sample_batch([points], [voxel_size], return_counts, return_trace, device)[0]
