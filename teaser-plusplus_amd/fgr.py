"""Fast Global Registration on the GPU with the surface of open3d.pipelines.registration:
FastGlobalRegistrationOption, registration_fgr_based_on_correspondence, registration_fgr_based_on_feature_matching,
plus a batched call and the per-iteration records as a stage call.  The contract is written out in
include/teaser_hip.h, "Fast Global Registration on correspondences": every sum has a fixed order, so a result does not
depend on the batch, the route (resident_max_corr) or the run."""
import ctypes as C

import numpy as np

from ._handles import HandleCache, _cloud, _get_option, _pairs, _per_problem, _rows, _set_option
from .icp import evaluate_registration_batch

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)

FLAG_FEW_CORRESPONDENCES, FLAG_ZERO_SCALE = 1, 2


class FgrParamsC(C.Structure):
    _fields_ = [("division_factor", C.c_double), ("maximum_correspondence_distance", C.c_double),
                ("use_absolute_scale", C.c_int32), ("decrease_mu", C.c_int32), ("iteration_number", C.c_int32),
                ("reserved", C.c_int32)]


class FgrResultC(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("optimised", C.c_double * 16), ("scale_global", C.c_double),
                ("scale_start", C.c_double), ("final_mu", C.c_double), ("iterations", C.c_int32),
                ("n_corr", C.c_int32), ("failed_solves", C.c_int32), ("flags", C.c_int32)]


assert C.sizeof(FgrParamsC) == 32 and C.sizeof(FgrResultC) == 296


def declare(L):
    """ctypes signatures of the FGR entry points (called by the package's lib())."""
    L.teaser_hip_fgr_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_fgr_destroy.argtypes = [_vp]
    L.teaser_hip_fgr_last_error.argtypes = [_vp]
    L.teaser_hip_fgr_last_error.restype = C.c_char_p
    L.teaser_hip_fgr_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_fgr_params_default.argtypes = [C.POINTER(FgrParamsC)]
    problems = [C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, C.POINTER(_ip), _ip, C.POINTER(FgrParamsC)]
    L.teaser_hip_fgr_correspondence_batch.argtypes = [_vp, C.c_int32] + problems + [C.POINTER(FgrResultC)]
    L.teaser_hip_fgr_correspondence.argtypes = [_vp, _dp, C.c_int32, _dp, C.c_int32, _ip, C.c_int32,
                                                C.POINTER(FgrParamsC), C.POINTER(FgrResultC)]
    L.teaser_hip_fgr_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
    L.teaser_hip_fgr_get_option.argtypes = [_vp, C.c_char_p, _i64p]
    L.teaser_hip_fgr_iterations_batch.argtypes = [_vp, C.c_int32] + problems + [C.c_int32, C.POINTER(FgrResultC), _dp,
                                                                                _dp, _dp, _dp, _ip, _dp, _dp, _dp]


_cache = HandleCache("teaser_hip_fgr")


class FastGlobalRegistrationOption:
    """Open3D's FastGlobalRegistrationOption, same fields and defaults, plus seed (the tuple test's draw; 0: from the
    clock).  maximum_tuple_count is NOT applied: the project's tuple test (tuple_test_batch) keeps every passing
    triple instead of stopping at a count."""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=True,
                 maximum_correspondence_distance=0.025, iteration_number=64, tuple_scale=0.95,
                 maximum_tuple_count=1000, tuple_test=True, seed=0):
        self.division_factor = float(division_factor)
        self.use_absolute_scale = bool(use_absolute_scale)
        self.decrease_mu = bool(decrease_mu)
        self.maximum_correspondence_distance = float(maximum_correspondence_distance)
        self.iteration_number = int(iteration_number)
        self.tuple_scale = float(tuple_scale)
        self.maximum_tuple_count = int(maximum_tuple_count)
        self.tuple_test = bool(tuple_test)
        self.seed = int(seed)

    def __repr__(self):
        return ("FastGlobalRegistrationOption(division_factor=%g, use_absolute_scale=%s, decrease_mu=%s, "
                "maximum_correspondence_distance=%g, iteration_number=%d, tuple_scale=%g, maximum_tuple_count=%d, "
                "tuple_test=%s, seed=%d)" % (self.division_factor, self.use_absolute_scale, self.decrease_mu,
                                             self.maximum_correspondence_distance, self.iteration_number,
                                             self.tuple_scale, self.maximum_tuple_count, self.tuple_test, self.seed))


def _params(option):
    if not isinstance(option, FastGlobalRegistrationOption):
        raise TypeError("option must be a FastGlobalRegistrationOption")
    p = FgrParamsC()
    p.division_factor = option.division_factor
    p.maximum_correspondence_distance = option.maximum_correspondence_distance
    p.use_absolute_scale = 1 if option.use_absolute_scale else 0
    p.decrease_mu = 1 if option.decrease_mu else 0
    p.iteration_number = option.iteration_number
    return p


def _gather(sources, targets, corres, option):
    b = len(sources)
    if len(targets) != b or len(corres) != b:
        raise ValueError("sources, targets and corres differ in length")
    src = [_cloud(a, "source %d" % k) for k, a in enumerate(sources)]
    dst = [_cloud(a, "target %d" % k) for k, a in enumerate(targets)]
    cor = [_pairs(a, "corres %d" % k) for k, a in enumerate(corres)]
    opts = [FastGlobalRegistrationOption() if o is None else o for o in _per_problem(option, b, "option")]
    params = (FgrParamsC * max(b, 1))()
    for k in range(b):
        params[k] = _params(opts[k])
    return b, src, dst, cor, opts, params


def _args(src, dst, cor, params):
    (sp, n_s), (dp, n_d), (cp, n_c) = _rows(src, _dp), _rows(dst, _dp), _rows(cor, _ip)
    return (sp, n_s.ctypes.data_as(_ip), dp, n_d.ctypes.data_as(_ip), cp, n_c.ctypes.data_as(_ip), params), (n_s, n_d, n_c)


def _tuple_filter(src, dst, cor, opts, device):
    """option.tuple_test: the batched tuple test on the pairs of the problems that ask for it."""
    which = [k for k, o in enumerate(opts) if o.tuple_test and len(cor[k]) > 0]
    if not which:
        return cor
    from .features import tuple_test_batch
    kept = tuple_test_batch([src[k] for k in which], [dst[k] for k in which], [cor[k] for k in which],
                            [opts[k].tuple_scale for k in which], [opts[k].seed for k in which], device)
    cor = list(cor)
    for k, a in zip(which, kept):
        cor[k] = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 2)
    return cor


def _record(rec):
    return dict(transformation=np.array(rec.transformation[:]).reshape(4, 4),
                optimised=np.array(rec.optimised[:]).reshape(4, 4), scale_global=float(rec.scale_global),
                scale_start=float(rec.scale_start), final_mu=float(rec.final_mu), iterations=int(rec.iterations),
                n_corr=int(rec.n_corr), failed_solves=int(rec.failed_solves), flags=int(rec.flags))


def registration_fgr_based_on_correspondence_batch(sources, targets, corres, option=None, device=-1):
    """registration_fgr_based_on_correspondence for lists of problems in one call: the list of results, each the bits
    the single call returns.  option: one FastGlobalRegistrationOption for all problems or a list with one per
    problem.  Each RegistrationResult is filled by evaluate_registration_batch at the FGR pose and
    maximum_correspondence_distance, as Open3D does, and carries the FGR record as .fgr (a dict: optimised,
    scale_global, scale_start, final_mu, iterations, n_corr, failed_solves, flags) and the pairs the solve ran on as
    .fgr_corres."""
    b, src, dst, cor, opts, params = _gather(sources, targets, corres, option)
    if b == 0:
        return []
    cor = _tuple_filter(src, dst, cor, opts, device)
    args, keep = _args(src, dst, cor, params)
    out = (FgrResultC * b)()
    h = _cache.get(device)
    h.call(h._lib.teaser_hip_fgr_correspondence_batch, b, *args, out)
    recs = [_record(out[k]) for k in range(b)]
    results = evaluate_registration_batch(src, dst, [o.maximum_correspondence_distance for o in opts],
                                          np.stack([r["transformation"] for r in recs]), device)
    for res, rec, c in zip(results, recs, cor):
        res.transformation = rec["transformation"]
        res.iterations = rec["iterations"]
        res.fgr = rec
        res.fgr_corres = c
    return results


def registration_fgr_based_on_correspondence(source, target, corres, option=None, device=-1):
    """Open3D's registration_fgr_based_on_correspondence (same argument order).  source / target: n x 3 points; corres:
    n x 2 (source index, target index).  With option.tuple_test (the default) the pairs first pass the tuple test."""
    return registration_fgr_based_on_correspondence_batch([source], [target], [corres], option, device)[0]


def registration_fgr_based_on_feature_matching(source, target, source_feature, target_feature, option=None, device=-1):
    """Open3D's registration_fgr_based_on_feature_matching (same argument order) composed on the device front-end: the
    mutual nearest-neighbour matches of the features (feature_matching_correspondences with the mutual filter, as the
    RANSAC form), the tuple test, then registration_fgr_based_on_correspondence.  The features are n x dim rows (what
    compute_fpfh_batch or compute_fpfh_feature returns), not Open3D's dim x n Feature.data."""
    from .ransac import feature_matching_correspondences
    pairs = feature_matching_correspondences(source_feature, target_feature, True, 3, device)
    return registration_fgr_based_on_correspondence(source, target, pairs, option, device)


def fgr_iterations_batch(sources, targets, corres, n, option=None, device=-1):
    """teaser_hip_fgr_iterations_batch: the first n iterations of every problem through the kernels and routes of the
    full call; the tuple test is NOT applied.  Per problem a dict: the full call's record after n steps
    (transformation, optimised, ...), mu (n), A (n x 6 x 6), g (n x 6), xi (n x 6), solve_flag (n), trans (n x 4 x 4),
    p (ncorr x 3) and q (ncorr x 3, the records after the n-th step)."""
    b, src, dst, cor, opts, params = _gather(sources, targets, corres, option)
    n = int(n)
    if b == 0:
        return []
    args, (n_s, n_d, n_c) = _args(src, dst, cor, params)
    m, tot = max(b * n, 1), max(int(n_c.sum()), 1)
    mu, A, g, xi = np.zeros(m), np.zeros((m, 36)), np.zeros((m, 6)), np.zeros((m, 6))
    flag, trans = np.zeros(m, dtype=np.int32), np.zeros((m, 16))
    p, q = np.zeros((tot, 3)), np.zeros((tot, 3))
    out = (FgrResultC * b)()
    h = _cache.get(device)
    h.call(h._lib.teaser_hip_fgr_iterations_batch, b, *args, n, out, mu.ctypes.data_as(_dp), A.ctypes.data_as(_dp),
           g.ctypes.data_as(_dp), xi.ctypes.data_as(_dp), flag.ctypes.data_as(_ip), trans.ctypes.data_as(_dp),
           p.ctypes.data_as(_dp), q.ctypes.data_as(_dp))
    res, first = [], 0
    for k in range(b):
        sl, pr = slice(k * n, (k + 1) * n), slice(first, first + int(n_c[k]))
        first += int(n_c[k])
        d = _record(out[k])
        d.update(mu=mu[sl].copy(), A=A[sl].reshape(-1, 6, 6).copy(), g=g[sl].copy(), xi=xi[sl].copy(),
                 solve_flag=flag[sl].copy(), trans=trans[sl].reshape(-1, 4, 4).copy(), p=p[pr].copy(), q=q[pr].copy())
        res.append(d)
    return res


def set_fgr_option(name, value, device=-1):
    """teaser_hip_fgr_set_option on the cached handle of `device` ("resident_max_corr" in 0 .. 3072: a tuning knob, no
    result bit depends on it)."""
    _set_option(_cache, name, value, device)


def get_fgr_option(name, device=-1):
    return _get_option(_cache, name, device)
