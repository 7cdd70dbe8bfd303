"""Voxel down-sampling on the GPU with Open3D's arithmetic (``pcd.voxel_down_sample(voxel_size)``):
``voxel_down_sample(points, voxel_size)`` and the batched ``voxel_down_sample_batch``.  The contract is written out in
include/teaser_hip.h ("Voxel down-sampling"): voxel index floor((p - (min_bound - v/2)) / v), output = FP64 mean of
the voxel's points summed in input order, voxels in ascending (i_x, i_y, i_z) order (Open3D's order is its hash
map's).

One library handle is kept per device between calls; calls from several threads are safe -- each handle has a lock,
so calls for one device run one after the other.  device=-1 means the calling thread's current HIP device at the
time of the call.  Without a GPU the calls raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import HandleCache, _cloud

_vp, _ip, _dp, _i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)


def declare(L):
    """ctypes signatures of the voxel entry points (called by the package's lib())."""
    L.teaser_hip_voxel_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_voxel_destroy.argtypes = [_vp]
    L.teaser_hip_voxel_last_error.argtypes = [_vp]
    L.teaser_hip_voxel_last_error.restype = C.c_char_p
    L.teaser_hip_voxel_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_voxel_down_sample_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, _dp, C.POINTER(_dp),
                                                     _i64p, C.POINTER(_ip), C.POINTER(_ip)]
    L.teaser_hip_voxel_down_sample.argtypes = [_vp, _dp, C.c_int32, C.c_double, _dp, _i64p, _ip, _ip]


_cache = HandleCache("teaser_hip_voxel")
_handle = _cache.get


def voxel_down_sample_batch(clouds, voxel_sizes, return_counts=False, return_trace=False, device=-1):
    """Down-samples many clouds (mixed sizes allowed) in one launch sequence.  voxel_sizes: one value for all clouds
    or one per cloud.  Returns a list with, per cloud, the n_out x 3 float64 voxel means -- or a tuple
    (means, counts, trace) with the parts asked for: counts[k] = points in voxel k, trace[i] = voxel of input point i.
    Each result is bit-identical to the same cloud down-sampled alone."""
    from . import lib
    pts = [_cloud(c, "points") for c in clouds]
    b = len(pts)
    vs = np.ascontiguousarray(np.broadcast_to(np.asarray(voxel_sizes, dtype=np.float64), (b,)))
    n = np.array([len(p) for p in pts], dtype=np.int32)
    outs = [np.empty((max(int(k), 1), 3)) for k in n]
    counts = [np.empty(max(int(k), 1), dtype=np.int32) for k in n] if return_counts else None
    trace = [np.empty(max(int(k), 1), dtype=np.int32) for k in n] if return_trace else None
    n_out = np.zeros(max(b, 1), dtype=np.int64)
    pp = (_dp * max(b, 1))(*[p.ctypes.data_as(_dp) for p in pts])
    op = (_dp * max(b, 1))(*[o.ctypes.data_as(_dp) for o in outs])
    cp = None if counts is None else (_ip * max(b, 1))(*[c.ctypes.data_as(_ip) for c in counts])
    tp = None if trace is None else (_ip * max(b, 1))(*[t.ctypes.data_as(_ip) for t in trace])
    _handle(device).call(lib().teaser_hip_voxel_down_sample_batch, b, pp, n.ctypes.data_as(_ip),
                         vs.ctypes.data_as(_dp), op, n_out.ctypes.data_as(_i64p), cp, tp)
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
