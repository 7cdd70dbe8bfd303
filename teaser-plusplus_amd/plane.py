"""Dominant-plane segmentation on the GPU with the surface of open3d.geometry.PointCloud.segment_plane, plus a batched
call and the per-trial records as a stage call.  The contract is written out in include/teaser_hip.h, "Plane
segmentation": trials are a function of (seed, trial index) alone, every sum has a fixed order and the loop is Open3D's
as one thread runs it, so a result does not depend on the batch, the launch sizes or the run."""
import ctypes as C
import math

import numpy as np

from ._handles import HandleCache, _cloud, _get_option, _per_problem, _rows, _set_option

_vp, _ip, _dp, _u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)

FLAG_VALID = 1


class PlaneParamsC(C.Structure):
    _fields_ = [("distance_threshold", C.c_double), ("ransac_n", C.c_int32), ("num_iterations", C.c_int32),
                ("probability", C.c_double), ("seed", C.c_uint64)]


class PlaneResultC(C.Structure):
    _fields_ = [("plane", C.c_double * 4), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("best_trial", C.c_int64), ("trials", C.c_int64), ("valid_trials", C.c_int64),
                ("n_inliers", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(PlaneParamsC) == 32 and C.sizeof(PlaneResultC) == 80


def declare(L):
    """ctypes signatures of the plane-segmentation entry points (called by the package's lib())."""
    L.teaser_hip_plane_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_plane_destroy.argtypes = [_vp]
    L.teaser_hip_plane_last_error.argtypes = [_vp]
    L.teaser_hip_plane_last_error.restype = C.c_char_p
    L.teaser_hip_plane_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_plane_params_default.argtypes = [C.POINTER(PlaneParamsC)]
    problems = [C.POINTER(_dp), _ip, C.POINTER(PlaneParamsC)]
    L.teaser_hip_plane_segment_batch.argtypes = [_vp, C.c_int32] + problems + [C.POINTER(PlaneResultC), C.POINTER(_ip),
                                                                               C.POINTER(_u8p)]
    L.teaser_hip_plane_segment.argtypes = [_vp, _dp, C.c_int32, C.POINTER(PlaneParamsC), C.POINTER(PlaneResultC), _ip,
                                           _u8p]
    L.teaser_hip_plane_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
    L.teaser_hip_plane_get_option.argtypes = [_vp, C.c_char_p, _i64p]
    L.teaser_hip_plane_trials_batch.argtypes = [_vp, C.c_int32] + problems + [C.c_int64, C.c_int32, _ip, _u8p, _dp, _ip,
                                                                              _dp]


_cache = HandleCache("teaser_hip_plane")


class PlaneSegmentation:
    """What segment_plane_batch returns per problem: plane_model (4), inliers (ascending int32 indices), mask (n bytes),
    fitness and inlier_rmse of the winning trial, best_trial (-1: none), trials and valid_trials."""

    def __init__(self, rec, inliers, mask):
        self.plane_model = np.array(rec.plane[:], dtype=np.float64)
        self.inliers = inliers[:rec.n_inliers].copy()
        self.mask = mask
        self.fitness, self.inlier_rmse = float(rec.fitness), float(rec.inlier_rmse)
        self.best_trial, self.trials, self.valid_trials = int(rec.best_trial), int(rec.trials), int(rec.valid_trials)

    def __repr__(self):
        return "PlaneSegmentation(plane_model=%s, %d inliers, fitness=%g, trials=%d)" % (
            self.plane_model.tolist(), len(self.inliers), self.fitness, self.trials)


def _params(distance_threshold, ransac_n, num_iterations, probability, seed, k=None):
    """One problem's parameters; the argument errors that need no device are raised here and name the argument."""
    where = "" if k is None else " (problem %d)" % k
    d, p = float(distance_threshold), float(probability)
    if not (math.isfinite(d) and d > 0):
        raise ValueError("distance_threshold must be finite and > 0%s" % where)
    if int(ransac_n) != ransac_n or not 3 <= int(ransac_n) <= 8:
        raise ValueError("ransac_n must be in 3 .. 8%s" % where)
    if int(num_iterations) != num_iterations or not 0 <= int(num_iterations) < 2 ** 31:
        raise ValueError("num_iterations must be an integer >= 0%s" % where)
    if not (p > 0 and p <= 1):
        raise ValueError("probability must be in (0, 1]%s" % where)
    q = PlaneParamsC()
    q.distance_threshold, q.ransac_n, q.num_iterations, q.probability = d, int(ransac_n), int(num_iterations), p
    q.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return q


def _gather(clouds, distance_threshold, ransac_n, num_iterations, probability, seed):
    b = len(clouds)
    pts = [_cloud(a, "points %d" % k) for k, a in enumerate(clouds)]
    for k, a in enumerate(pts):
        if not np.isfinite(a).all():
            raise ValueError("points %d has non-finite points" % k)
    ds, ns, its, prs, seeds = (_per_problem(v, b, w) for v, w in (
        (distance_threshold, "distance_threshold"), (ransac_n, "ransac_n"), (num_iterations, "num_iterations"),
        (probability, "probability"), (seed, "seed")))
    params = (PlaneParamsC * max(b, 1))()
    for k in range(b):
        params[k] = _params(ds[k], ns[k], its[k], prs[k], seeds[k], k)
    pp, n = _rows(pts, _dp)
    return b, (pp, n.ctypes.data_as(_ip), params), (pts, n)


def segment_plane_batch(clouds, distance_threshold, ransac_n=3, num_iterations=100, probability=0.99999999, seed=0,
                        device=-1):
    """segment_plane for a list of clouds in one call: a list of PlaneSegmentation, each the bits the single call
    returns.  distance_threshold, ransac_n, num_iterations, probability and seed: one value for all problems or a list
    with one per problem."""
    b, args, keep = _gather(clouds, distance_threshold, ransac_n, num_iterations, probability, seed)
    if b == 0:
        return []
    out = (PlaneResultC * b)()
    inl = [np.zeros(max(len(a), 1), dtype=np.int32) for a in keep[0]]
    msk = [np.zeros(max(len(a), 1), dtype=np.uint8) for a in keep[0]]
    ip = (_ip * b)(*[a.ctypes.data_as(_ip) for a in inl])
    mp = (_u8p * b)(*[a.ctypes.data_as(_u8p) for a in msk])
    h = _cache.get(device)
    h.call(h._lib.teaser_hip_plane_segment_batch, b, *args, out, ip, mp)
    return [PlaneSegmentation(out[k], inl[k], msk[k][:len(keep[0][k])].copy()) for k in range(b)]


def segment_plane(points, distance_threshold, ransac_n=3, num_iterations=100, probability=0.99999999, seed=0,
                  device=-1):
    """Open3D's PointCloud.segment_plane (same argument order) on an n x 3 array, plus the seed: 0 draws from the clock,
    any other value is reproducible.  Returns (plane_model[4], inliers): a x + b y + c z + d = 0 and the ascending
    indices within distance_threshold of the winning trial's plane."""
    r = segment_plane_batch([points], distance_threshold, ransac_n, num_iterations, probability, seed, device)[0]
    return r.plane_model, r.inliers


def plane_trials_batch(clouds, distance_threshold, first, n, ransac_n=3, seed=0, device=-1):
    """teaser_hip_plane_trials_batch: trials first .. first + n - 1 of every problem through the kernels of the full
    call, no stopping rule.  Per problem a dict: samples (n x ransac_n), flags (n, bit FLAG_VALID), plane (n x 4),
    count (n), E (n)."""
    b, args, keep = _gather(clouds, distance_threshold, ransac_n, 0, 1.0, seed)
    first, n = int(first), int(n)
    if b == 0:
        return []
    m = max(b * n, 1)
    samples, flags = np.zeros((m, 8), dtype=np.int32), np.zeros(m, dtype=np.uint8)
    planes, count, E = np.zeros((m, 4)), np.zeros(m, dtype=np.int32), np.zeros(m)
    h = _cache.get(device)
    h.call(h._lib.teaser_hip_plane_trials_batch, b, *args, first, n, samples.ctypes.data_as(_ip),
           flags.ctypes.data_as(_u8p), planes.ctypes.data_as(_dp), count.ctypes.data_as(_ip), E.ctypes.data_as(_dp))
    out = []
    for k in range(b):
        sl = slice(k * n, (k + 1) * n)
        out.append(dict(samples=samples[sl, :args[2][k].ransac_n].copy(), flags=flags[sl].copy(),
                        plane=planes[sl].copy(), count=count[sl].copy(), E=E[sl].copy()))
    return out


def set_plane_option(name, value, device=-1):
    """teaser_hip_plane_set_option on the cached handle of `device` ("chunk_trials", "partial_bytes": tuning knobs, no
    result bit depends on them)."""
    _set_option(_cache, name, value, device)


def get_plane_option(name, device=-1):
    return _get_option(_cache, name, device)
