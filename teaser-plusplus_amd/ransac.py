"""RANSAC registration on the GPU with the surface of open3d.pipelines.registration:
registration_ransac_based_on_correspondence, registration_ransac_based_on_feature_matching, RANSACConvergenceCriteria,
CorrespondenceCheckerBasedOnEdgeLength and CorrespondenceCheckerBasedOnDistance, plus a batched call and the per-trial
records as a stage call.  The contract is written out in include/teaser_hip.h, "RANSAC registration on correspondences":
trials are a function of (seed, trial index) alone and the loop is Open3D's as one thread runs it, so a result does not
depend on the batch, the launch sizes or the run."""
import ctypes as C

import numpy as np

from ._handles import HandleCache, _cloud, _get_option, _pairs, _per_problem, _rows, _set_option
from .icp import RegistrationResult, TransformationEstimationPointToPoint

_vp, _ip, _dp, _u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)

FLAG_EDGE_LENGTH, FLAG_DISTANCE, FLAG_SCORED = 1, 2, 4


class RansacParamsC(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("ransac_n", C.c_int32), ("max_iteration", C.c_int32),
                ("confidence", C.c_double), ("seed", C.c_uint64), ("edge_length_threshold", C.c_double),
                ("distance_threshold", C.c_double), ("with_scaling", C.c_int32), ("estimation", C.c_int32),
                ("normal_checker", C.c_int32), ("reserved", C.c_int32)]


class RansacResultC(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("best_trial", C.c_int64), ("trials", C.c_int64), ("valid_trials", C.c_int64),
                ("n_correspondences", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(RansacParamsC) == 64 and C.sizeof(RansacResultC) == 176


def declare(L):
    """ctypes signatures of the RANSAC entry points (called by the package's lib())."""
    L.teaser_hip_ransac_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_ransac_destroy.argtypes = [_vp]
    L.teaser_hip_ransac_last_error.argtypes = [_vp]
    L.teaser_hip_ransac_last_error.restype = C.c_char_p
    L.teaser_hip_ransac_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_ransac_params_default.argtypes = [C.POINTER(RansacParamsC)]
    problems = [C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, C.POINTER(_ip), _ip, C.POINTER(RansacParamsC)]
    L.teaser_hip_ransac_correspondence_batch.argtypes = [_vp, C.c_int32] + problems + [C.POINTER(RansacResultC),
                                                                                       C.POINTER(_ip)]
    L.teaser_hip_ransac_correspondence.argtypes = [_vp, _dp, C.c_int32, _dp, C.c_int32, _ip, C.c_int32,
                                                   C.POINTER(RansacParamsC), C.POINTER(RansacResultC), _ip]
    L.teaser_hip_ransac_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
    L.teaser_hip_ransac_get_option.argtypes = [_vp, C.c_char_p, _i64p]
    L.teaser_hip_ransac_trials_batch.argtypes = [_vp, C.c_int32] + problems + [C.c_int64, C.c_int32, _ip, _u8p, _dp,
                                                                               _ip, _dp]


_cache = HandleCache("teaser_hip_ransac")


class RANSACConvergenceCriteria:
    """Open3D's RANSACConvergenceCriteria (max_iteration 100000, confidence 0.999)."""

    def __init__(self, max_iteration=100000, confidence=0.999):
        self.max_iteration, self.confidence = int(max_iteration), float(confidence)

    def __repr__(self):
        return "RANSACConvergenceCriteria(max_iteration=%d, confidence=%g)" % (self.max_iteration, self.confidence)


class CorrespondenceCheckerBasedOnEdgeLength:
    """Open3D's checker: every pair of sampled correspondences keeps its length within the factor
    similarity_threshold in (0, 1] between the clouds."""

    def __init__(self, similarity_threshold=0.9):
        self.similarity_threshold = float(similarity_threshold)


class CorrespondenceCheckerBasedOnDistance:
    """Open3D's checker: every sampled correspondence lies within distance_threshold under the estimate."""

    def __init__(self, distance_threshold):
        self.distance_threshold = float(distance_threshold)


class CorrespondenceCheckerBasedOnNormal:
    """Open3D's normal-angle checker: NOT offered; passing one is an argument error that names it."""

    def __init__(self, normal_angle_threshold):
        self.normal_angle_threshold = float(normal_angle_threshold)


def _params(max_correspondence_distance, estimation_method, ransac_n, checkers, criteria, seed):
    p = RansacParamsC()
    from . import lib
    lib().teaser_hip_ransac_params_default(C.byref(p))
    p.max_correspondence_distance = float(max_correspondence_distance)
    if estimation_method is not None and not isinstance(estimation_method, TransformationEstimationPointToPoint):
        if getattr(estimation_method, "with_scaling", False):
            raise ValueError("estimation_method: with_scaling=True is not offered")
        raise ValueError("estimation_method: only TransformationEstimationPointToPoint(with_scaling=False) is offered "
                         "inside RANSAC (point-to-plane estimation is not), got %s" % type(estimation_method).__name__)
    p.ransac_n = int(ransac_n)
    criteria = RANSACConvergenceCriteria() if criteria is None else criteria
    if not isinstance(criteria, RANSACConvergenceCriteria):
        raise TypeError("criteria must be a RANSACConvergenceCriteria")
    p.max_iteration, p.confidence = criteria.max_iteration, criteria.confidence
    p.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seen = set()
    for ch in checkers or ():
        if isinstance(ch, CorrespondenceCheckerBasedOnEdgeLength):
            kind, field, value = "edge length", "edge_length_threshold", ch.similarity_threshold
        elif isinstance(ch, CorrespondenceCheckerBasedOnDistance):
            kind, field, value = "distance", "distance_threshold", ch.distance_threshold
        elif isinstance(ch, CorrespondenceCheckerBasedOnNormal):
            raise ValueError("checkers: the normal-angle checker (CorrespondenceCheckerBasedOnNormal) is not offered")
        else:
            raise TypeError("checkers: %r is not a CorrespondenceChecker" % (ch,))
        if kind in seen:
            raise ValueError("checkers: more than one %s checker" % kind)
        seen.add(kind)
        if not value > 0:  # 0 would mean "off" to the C ABI: a checker that is given must be on
            raise ValueError("checkers: the %s threshold must be > 0" % kind)
        setattr(p, field, value)
    return p


def _gather(sources, targets, corres, max_correspondence_distance, estimation_method, ransac_n, checkers, criteria,
            seed):
    b = len(sources)
    if len(targets) != b or len(corres) != b:
        raise ValueError("sources, targets and corres differ in length")
    src = [_cloud(a, "source %d" % k) for k, a in enumerate(sources)]
    dst = [_cloud(a, "target %d" % k) for k, a in enumerate(targets)]
    cor = [_pairs(a, "corres %d" % k) for k, a in enumerate(corres)]
    rs, ns, crit, seeds = (_per_problem(v, b, w) for v, w in (
        (max_correspondence_distance, "max_correspondence_distance"), (ransac_n, "ransac_n"), (criteria, "criteria"),
        (seed, "seed")))
    if checkers and all(isinstance(c, (list, tuple)) for c in checkers):  # one list of checkers per problem
        if len(checkers) != b:
            raise ValueError("checkers: %d lists for %d problems" % (len(checkers), b))
        chk = list(checkers)
    else:
        chk = [checkers] * b
    params = (RansacParamsC * max(b, 1))()
    for k in range(b):
        params[k] = _params(rs[k], estimation_method, ns[k], chk[k], crit[k], seeds[k])
    (sp, n_s), (dp, n_d), (cp, n_c) = _rows(src, _dp), _rows(dst, _dp), _rows(cor, _ip)
    keep = (src, dst, cor, n_s, n_d, n_c)
    return b, (sp, n_s.ctypes.data_as(_ip), dp, n_d.ctypes.data_as(_ip), cp, n_c.ctypes.data_as(_ip), params), keep


def _result(rec, inliers):
    res = RegistrationResult(np.array(rec.transformation[:], dtype=np.float64).reshape(4, 4), float(rec.fitness),
                             float(rec.inlier_rmse), inliers[:rec.n_correspondences].copy(), int(rec.trials))
    res.best_trial, res.trials, res.valid_trials = int(rec.best_trial), int(rec.trials), int(rec.valid_trials)
    return res


def registration_ransac_based_on_correspondence_batch(sources, targets, corres, max_correspondence_distance,
                                                      estimation_method=None, ransac_n=3, checkers=(), criteria=None,
                                                      seed=0, device=-1):
    """registration_ransac_based_on_correspondence for lists of problems in one call: the list of results, each the
    bits the single call returns.  max_correspondence_distance, ransac_n, criteria and seed: one value for all problems
    or a list with one per problem; checkers: one list for all problems or a list of lists."""
    b, args, keep = _gather(sources, targets, corres, max_correspondence_distance, estimation_method, ransac_n,
                            checkers, criteria, seed)
    if b == 0:
        return []
    out = (RansacResultC * b)()
    inl = [np.zeros((max(len(c), 1), 2), dtype=np.int32) for c in keep[2]]
    ip = (_ip * b)(*[a.ctypes.data_as(_ip) for a in inl])
    h = _cache.get(device)
    h.call(h._lib.teaser_hip_ransac_correspondence_batch, b, *args, out, ip)
    return [_result(out[k], inl[k]) for k in range(b)]


def registration_ransac_based_on_correspondence(source, target, corres, max_correspondence_distance,
                                                estimation_method=None, ransac_n=3, checkers=(), criteria=None,
                                                seed=0, device=-1):
    """Open3D's registration_ransac_based_on_correspondence (same argument order).  source / target: n x 3 points;
    corres: n x 2 (source index, target index).  seed: 0 draws from the clock, any other value is reproducible.  Returns
    a RegistrationResult (correspondence_set = the inlier pairs in input order) with best_trial, trials and
    valid_trials added."""
    return registration_ransac_based_on_correspondence_batch([source], [target], [corres], max_correspondence_distance,
                                                             estimation_method, ransac_n, checkers, criteria, seed,
                                                             device)[0]


def feature_matching_correspondences(source_feature, target_feature, mutual_filter, ransac_n=3, device=-1):
    """The correspondences registration_ransac_based_on_feature_matching runs on: (i, j) with j the nearest target
    feature of source row i (match_features_knn_batch, k = 1, mutual=False); with mutual_filter only the pairs whose
    reverse match agrees, unless fewer than ransac_n survive: then all pairs, as Open3D does."""
    from .features import match_features_knn_batch
    sets = [source_feature, target_feature] if mutual_filter else [source_feature]
    other = [target_feature, source_feature] if mutual_filter else [target_feature]
    found = match_features_knn_batch(sets, other, 1, False, device)
    pairs = found[0]
    if mutual_filter:
        back = np.full(len(np.asarray(target_feature)), -1, dtype=np.int64)
        back[found[1][:, 0]] = found[1][:, 1]
        kept = pairs[back[pairs[:, 1]] == pairs[:, 0]]
        if len(kept) >= int(ransac_n):
            pairs = kept
    return np.ascontiguousarray(pairs, dtype=np.int32)


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter,
                                                  max_correspondence_distance, estimation_method=None, ransac_n=3,
                                                  checkers=(), criteria=None, seed=0, device=-1):
    """Open3D's registration_ransac_based_on_feature_matching (same argument order) composed on the device front-end:
    feature_matching_correspondences, then registration_ransac_based_on_correspondence.  The features are n x dim rows
    (what compute_fpfh_batch or compute_fpfh_feature returns), not Open3D's dim x n Feature.data."""
    pairs = feature_matching_correspondences(source_feature, target_feature, mutual_filter, ransac_n, device)
    return registration_ransac_based_on_correspondence(source, target, pairs, max_correspondence_distance,
                                                       estimation_method, ransac_n, checkers, criteria, seed, device)


def ransac_trials_batch(sources, targets, corres, max_correspondence_distance, first, n, estimation_method=None,
                        ransac_n=3, checkers=(), seed=0, device=-1):
    """teaser_hip_ransac_trials_batch: trials first .. first + n - 1 of every problem through the kernels of the full
    call, no stopping rule.  Per problem a dict: samples (n x ransac_n), flags (n, bits FLAG_*), transformation
    (n x 4 x 4), count (n), sum_d2 (n)."""
    b, args, keep = _gather(sources, targets, corres, max_correspondence_distance, estimation_method, ransac_n,
                            checkers, None, seed)
    first, n = int(first), int(n)
    if b == 0:
        return []
    m = max(b * n, 1)
    samples, flags = np.zeros((m, 8), dtype=np.int32), np.zeros(m, dtype=np.uint8)
    T, count, sums = np.zeros((m, 16)), np.zeros(m, dtype=np.int32), np.zeros(m)
    h = _cache.get(device)
    h.call(h._lib.teaser_hip_ransac_trials_batch, b, *args, first, n, samples.ctypes.data_as(_ip),
           flags.ctypes.data_as(_u8p), T.ctypes.data_as(_dp), count.ctypes.data_as(_ip), sums.ctypes.data_as(_dp))
    out = []
    for k in range(b):
        sl = slice(k * n, (k + 1) * n)
        out.append(dict(samples=samples[sl, :args[6][k].ransac_n].copy(), flags=flags[sl].copy(),
                        transformation=T[sl].reshape(-1, 4, 4).copy(), count=count[sl].copy(), sum_d2=sums[sl].copy()))
    return out


def set_ransac_option(name, value, device=-1):
    """teaser_hip_ransac_set_option on the cached handle of `device` ("chunk_trials": a tuning knob, no result bit
    depends on it)."""
    _set_option(_cache, name, value, device)


def get_ransac_option(name, device=-1):
    return _get_option(_cache, name, device)
