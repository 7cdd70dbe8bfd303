"""ICP refinement on the GPU with Open3D's interface (``o3d.pipelines.registration``):
``registration_icp(source, target, max_correspondence_distance, init, estimation_method, criteria)`` and the batched
``registration_icp_batch``.  The semantics are those of Open3D's RegistrationICP with
TransformationEstimationPointToPoint(with_scaling=False) or TransformationEstimationPointToPlane(kernel) (target
normals given by the caller, robust kernels L2 / Huber / Cauchy / GM / Tukey) or the formulation of
TransformationEstimationForGeneralizedICP (per-point covariances of both clouds, L2 only; ``estimate_covariances``
computes them on the GPU) or of TransformationEstimationForColoredICP (colours of both clouds and target normals;
``registration_colored_icp``), written out in include/teaser_hip.h ("ICP refinement").

One library handle is kept per device between calls (no HIP context per call); calls from several threads are safe --
each handle has a lock, so calls for one device run one after the other.  device=-1 means the calling thread's
current HIP device at the time of the call.  Without a GPU the calls raise
TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C

import numpy as np

from ._handles import HandleCache, _cloud

_vp, _ip, _dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)


class IcpParamsC(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("max_iteration", C.c_int32),
                ("relative_fitness", C.c_double), ("relative_rmse", C.c_double)]


class IcpResultC(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("iterations", C.c_int32), ("n_correspondences", C.c_int32)]


class IcpEstimationC(C.Structure):
    _fields_ = [("method", C.c_int32), ("kernel", C.c_int32), ("kernel_k", C.c_double)]


class IcpNormalSearchC(C.Structure):
    _fields_ = [("search", C.c_int32), ("max_nn", C.c_int32), ("radius", C.c_double), ("orient", C.c_int32),
                ("reserved", C.c_int32), ("ref", C.c_double * 3)]


assert C.sizeof(IcpNormalSearchC) == 48  # teaser_icp_normal_search_c: the header asserts the same


class IcpColorC(C.Structure):
    _fields_ = [("lambda_geometric", C.c_double), ("gradient_radius", C.c_double), ("gradient_max_nn", C.c_int32),
                ("reserved", C.c_int32)]


assert C.sizeof(IcpColorC) == 24  # teaser_icp_color_c: the header asserts the same


def declare(L):
    """ctypes signatures of the ICP entry points (called by the package's lib())."""
    L.teaser_hip_icp_params_default.argtypes = [C.POINTER(IcpParamsC)]
    L.teaser_hip_icp_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_icp_destroy.argtypes = [_vp]
    L.teaser_hip_icp_last_error.argtypes = [_vp]
    L.teaser_hip_icp_last_error.restype = C.c_char_p
    L.teaser_hip_icp_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_icp_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, _dp,
                                       C.POINTER(IcpParamsC), C.POINTER(IcpResultC), C.POINTER(_ip)]
    L.teaser_hip_icp_solve.argtypes = [_vp, _dp, C.c_int32, _dp, C.c_int32, _dp, C.POINTER(IcpParamsC),
                                       C.POINTER(IcpResultC), _ip]
    L.teaser_hip_icp_estimation_default.argtypes = [C.POINTER(IcpEstimationC)]
    L.teaser_hip_icp_batch_ex.argtypes = L.teaser_hip_icp_batch.argtypes + [C.POINTER(_dp), C.POINTER(IcpEstimationC)]
    L.teaser_hip_icp_solve_ex.argtypes = L.teaser_hip_icp_solve.argtypes + [_dp, C.POINTER(IcpEstimationC)]
    L.teaser_hip_icp_batch_cov.argtypes = L.teaser_hip_icp_batch_ex.argtypes + [C.POINTER(_dp), C.POINTER(_dp)]
    L.teaser_hip_icp_solve_cov.argtypes = L.teaser_hip_icp_solve_ex.argtypes + [_dp, _dp]
    L.teaser_hip_icp_covariances_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, _dp, _ip, _dp, C.POINTER(_dp)]
    L.teaser_hip_icp_normals_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(IcpNormalSearchC),
                                               C.POINTER(_dp), C.POINTER(_dp), C.POINTER(_dp)]
    L.teaser_hip_icp_batch_auto.argtypes = L.teaser_hip_icp_batch_cov.argtypes + [C.POINTER(IcpNormalSearchC)]
    L.teaser_hip_icp_solve_auto.argtypes = L.teaser_hip_icp_solve_cov.argtypes + [C.POINTER(IcpNormalSearchC)]
    L.teaser_hip_icp_color_default.argtypes = [C.POINTER(IcpColorC)]
    L.teaser_hip_icp_batch_color.argtypes = L.teaser_hip_icp_batch_cov.argtypes + [C.POINTER(_dp), C.POINTER(_dp),
                                                                                   C.POINTER(_dp), C.POINTER(IcpColorC)]
    L.teaser_hip_icp_solve_color.argtypes = L.teaser_hip_icp_solve_cov.argtypes + [_dp, _dp, _dp, C.POINTER(IcpColorC)]
    L.teaser_hip_icp_color_gradients_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(_dp),
                                                       C.POINTER(_dp), _dp, _ip, C.POINTER(_dp)]
    L.teaser_hip_icp_information_batch.argtypes = [_vp, C.c_int32, C.POINTER(_dp), _ip, C.POINTER(_dp), _ip, _dp, _dp,
                                                   _dp, C.POINTER(IcpResultC), C.POINTER(_ip)]
    L.teaser_hip_icp_information.argtypes = [_vp, _dp, C.c_int32, _dp, C.c_int32, _dp, C.c_double, _dp,
                                             C.POINTER(IcpResultC), _ip]


class ICPConvergenceCriteria:
    """Open3D's ICPConvergenceCriteria: the loop stops when BOTH the fitness and the inlier RMSE changed by less
    than these ABSOLUTE amounts in one iteration, or after max_iteration iterations."""

    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness = float(relative_fitness)
        self.relative_rmse = float(relative_rmse)
        self.max_iteration = int(max_iteration)

    def __repr__(self):
        return "ICPConvergenceCriteria(relative_fitness=%g, relative_rmse=%g, max_iteration=%d)" % (
            self.relative_fitness, self.relative_rmse, self.max_iteration)


class TransformationEstimationPointToPoint:
    """Open3D's point-to-point estimation; only with_scaling=False exists here."""

    def __init__(self, with_scaling=False):
        if with_scaling:
            raise ValueError("TransformationEstimationPointToPoint(with_scaling=True) is not supported")
        self.with_scaling = False


class _RobustKernel:
    """Open3D's RobustKernel: the weight w(r) a point-to-plane residual r enters the normal equations with."""
    code = 0

    def __init__(self, k=1.0):
        self.k = float(k)

    def __repr__(self):
        return "%s(k=%g)" % (type(self).__name__, self.k)


class L2Loss(_RobustKernel):
    """w = 1 (no parameter)."""

    def __init__(self):
        super().__init__(1.0)

    def __repr__(self):
        return "L2Loss()"


class HuberLoss(_RobustKernel):
    """w = 1 if |r| <= k else k / |r|."""
    code = 1


class CauchyLoss(_RobustKernel):
    """w = 1 / (1 + (r / k)^2)."""
    code = 2


class GMLoss(_RobustKernel):
    """w = k / (k + r^2)^2."""
    code = 3


class TukeyLoss(_RobustKernel):
    """w = (1 - (r / k)^2)^2 if |r| <= k else 0."""
    code = 4


class TransformationEstimationPointToPlane:
    """Open3D's point-to-plane estimation with an optional robust kernel (default L2Loss).  The target normals are
    given to registration_icp(..., target_normals=...)."""

    def __init__(self, kernel=None):
        kernel = L2Loss() if kernel is None else kernel
        if not isinstance(kernel, _RobustKernel):
            raise ValueError("kernel must be L2Loss, HuberLoss, CauchyLoss, GMLoss or TukeyLoss")
        self.kernel = kernel


class TransformationEstimationForGeneralizedICP:
    """Open3D's Generalized-ICP estimation (plane-to-plane), L2 only: Open3D's robust kernels weight the whitened
    residual, which is not offered here, so a kernel other than None / L2Loss is refused.  The covariances of both
    clouds are given to registration_icp(..., source_covariances=..., target_covariances=...); epsilon is the value
    estimate_covariances is called with when registration_generalized_icp computes them."""

    def __init__(self, epsilon=1e-3, kernel=None):
        if kernel is not None and not isinstance(kernel, L2Loss):
            raise ValueError("TransformationEstimationForGeneralizedICP: only the L2 kernel is supported")
        epsilon = float(epsilon)
        if not (np.isfinite(epsilon) and epsilon > 0):
            raise ValueError("epsilon must be finite and > 0")
        self.epsilon = epsilon
        self.kernel = L2Loss()


MAX_NN_LIMIT = 100  # TEASER_HIP_ICP_COV_MAX_NN


class TransformationEstimationForColoredICP:
    """Open3D's Colored-ICP estimation (Park, Zhou, Koltun, ICCV 2017): the joint geometric + photometric objective,
    lambda_geometric the weight of the geometric term, with an optional robust kernel applied to both residuals
    (default L2Loss).  The colours and the target normals are given to registration_colored_icp / registration_icp;
    gradient_radius (None: twice max_correspondence_distance) and gradient_max_nn choose the neighbourhood the target's
    colour gradients are estimated from."""

    def __init__(self, lambda_geometric=0.968, kernel=None, gradient_radius=None, gradient_max_nn=30):
        kernel = L2Loss() if kernel is None else kernel
        if not isinstance(kernel, _RobustKernel):
            raise ValueError("kernel must be L2Loss, HuberLoss, CauchyLoss, GMLoss or TukeyLoss")
        lambda_geometric = float(lambda_geometric)
        if not (np.isfinite(lambda_geometric) and 0.0 <= lambda_geometric <= 1.0):
            raise ValueError("lambda_geometric must lie in [0, 1]")
        if gradient_radius is not None and not (np.isfinite(gradient_radius) and gradient_radius > 0):
            raise ValueError("gradient_radius must be finite and > 0")
        if not 4 <= int(gradient_max_nn) <= MAX_NN_LIMIT:
            raise ValueError("gradient_max_nn must lie in [4, %d]" % MAX_NN_LIMIT)
        self.lambda_geometric = lambda_geometric
        self.kernel = kernel
        self.gradient_radius = None if gradient_radius is None else float(gradient_radius)
        self.gradient_max_nn = int(gradient_max_nn)

    def record(self):
        return IcpColorC(self.lambda_geometric, 0.0 if self.gradient_radius is None else self.gradient_radius,
                         self.gradient_max_nn, 0)


class RegistrationResult:
    """Open3D's RegistrationResult (transformation, fitness, inlier_rmse, correspondence_set) + iterations."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondence_set, iterations):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.correspondence_set = correspondence_set
        self.iterations = iterations

    def __repr__(self):
        return "RegistrationResult(fitness=%.6g, inlier_rmse=%.6g, correspondences=%d, iterations=%d)" % (
            self.fitness, self.inlier_rmse, len(self.correspondence_set), self.iterations)


_cache = HandleCache("teaser_hip_icp")
_handle = _cache.get


class _NormalSearch:
    """A neighbourhood for normal estimation, optionally with an orientation: ``.towards(point)`` (Open3D's
    orient_normals_towards_camera_location) or ``.along(direction)`` (orient_normals_to_align_with_direction) return
    a copy with that orientation."""
    search = 0

    def __init__(self, radius, max_nn):
        self.radius, self.max_nn = float(radius), int(max_nn)
        self.orient, self.ref = 0, (0.0, 0.0, 0.0)
        if not 3 <= self.max_nn <= MAX_NN_LIMIT:
            raise ValueError("max_nn / knn must lie in [3, %d]" % MAX_NN_LIMIT)

    def _oriented(self, orient, ref, what):
        v = np.asarray(ref, dtype=np.float64).ravel()
        if v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError("%s must be 3 finite numbers" % what)
        out = type(self).__new__(type(self))
        out.__dict__.update(self.__dict__)
        out.orient, out.ref = orient, tuple(float(x) for x in v)
        return out

    def towards(self, point):
        return self._oriented(1, point, "towards")

    def along(self, direction):
        return self._oriented(2, direction, "along")

    def record(self):
        return IcpNormalSearchC(self.search, self.max_nn, self.radius, self.orient, 0, (C.c_double * 3)(*self.ref))


class KDTreeSearchParamHybrid(_NormalSearch):
    """Open3D's KDTreeSearchParamHybrid(radius, max_nn): the max_nn nearest neighbours inside radius."""
    search = 0

    def __init__(self, radius, max_nn):
        super().__init__(radius, max_nn)
        if not (np.isfinite(self.radius) and self.radius > 0):
            raise ValueError("radius must be finite and > 0")

    def __repr__(self):
        return "KDTreeSearchParamHybrid(radius=%g, max_nn=%d)" % (self.radius, self.max_nn)


class KDTreeSearchParamKNN(_NormalSearch):
    """Open3D's KDTreeSearchParamKNN(knn): the knn nearest neighbours, no radius.  (KDTreeSearchParamRadius, a radius
    without a cap, is not offered: include/teaser_hip.h, "Normal estimation".)"""
    search = 1

    def __init__(self, knn=30):
        super().__init__(0.0, knn)
        self.knn = self.max_nn

    def __repr__(self):
        return "KDTreeSearchParamKNN(knn=%d)" % self.max_nn


def _points(a, what):
    return _cloud(a, what, kind="array of points")


def _init(T):
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    if T.shape != (4, 4):
        raise ValueError("init must be 4 x 4, got shape %s" % (T.shape,))
    return T


def _params(r, criteria):
    c = criteria if criteria is not None else ICPConvergenceCriteria()
    return IcpParamsC(float(r), int(c.max_iteration), float(c.relative_fitness), float(c.relative_rmse))


def _estimation(m):
    """(method, kernel, k) codes of one estimation method; None is point-to-point."""
    if m is None or isinstance(m, TransformationEstimationPointToPoint):
        return 0, 0, 1.0
    if isinstance(m, TransformationEstimationPointToPlane):
        return 1, m.kernel.code, m.kernel.k
    if isinstance(m, TransformationEstimationForGeneralizedICP):
        return 2, 0, 1.0
    if isinstance(m, TransformationEstimationForColoredICP):
        return 3, m.kernel.code, m.kernel.k
    raise ValueError("estimation_method must be TransformationEstimationPointToPoint(with_scaling=False), "
                     "TransformationEstimationPointToPlane(kernel), TransformationEstimationForGeneralizedICP() or "
                     "TransformationEstimationForColoredICP()")


def _covariances(a, n, what, k):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if a.size == 0 and n == 0:
        return np.zeros((0, 3, 3))
    if a.shape not in ((n, 3, 3), (n, 9)):
        raise ValueError("%s must be %d x 3 x 3 (or %d x 9), got shape %s (problem %d)" % (what, n, n, a.shape, k))
    return a.reshape(n, 3, 3)


def _per_problem_covariances(given, ests, clouds, what):
    """One n x 3 x 3 array per Generalized-ICP problem (None elsewhere); ValueError when one is missing."""
    b = len(ests)
    out = [None] * b
    if not any(m[0] == 2 for m in ests):
        return out
    if given is None or len(given) != b:
        raise ValueError("Generalized ICP needs %s: one entry per problem" % what)
    for k in range(b):
        if ests[k][0] != 2:
            continue
        if given[k] is None:
            raise ValueError("Generalized ICP needs %s (problem %d)" % (what, k))
        out[k] = _covariances(given[k], len(clouds[k]), what, k)
    return out


def _per_problem_rows(given, ests, clouds, what, required=True):
    """One n x 3 array per Colored-ICP problem (None elsewhere, or where an optional one is not given)."""
    b = len(ests)
    out = [None] * b
    if not any(m[0] == 3 for m in ests):
        return out
    if given is None or len(given) != b:
        if not required and given is None:
            return out
        raise ValueError("Colored ICP needs %s: one entry per problem" % what)
    for k in range(b):
        if ests[k][0] != 3:
            continue
        if given[k] is None:
            if required:
                raise ValueError("Colored ICP needs %s (problem %d)" % (what, k))
            continue
        a = _points(given[k], what)
        if a.shape != clouds[k].shape:
            raise ValueError("%s must have the cloud's shape %s, got %s (problem %d)"
                             % (what, clouds[k].shape, a.shape, k))
        out[k] = a
    return out


def registration_icp_batch(sources, targets, max_correspondence_distance, inits=None, criteria=None, device=-1,
                           estimation_methods=None, target_normals=None, source_covariances=None,
                           target_covariances=None, *, source_colors=None, target_colors=None,
                           target_color_gradients=None):
    """One launch sequence for many independent problems (mixed sizes allowed).  max_correspondence_distance and
    criteria: one value for all or one per problem; inits: None (identity), one 4 x 4 for all, or one per problem;
    estimation_methods: None (point-to-point), one for all or one per problem; target_normals: None, or one entry per
    problem (None for a point-to-point problem, else one normal per target point, or a KDTreeSearchParamHybrid /
    KDTreeSearchParamKNN object: the normals are then estimated from the target on the device); source_covariances /
    target_covariances: None, or one entry per problem (None unless the problem is Generalized ICP, else n x 3 x 3);
    source_colors / target_colors: None, or one entry per problem (None unless the problem is Colored ICP, else n x 3
    colours; such a problem also needs its target normals as an array); target_color_gradients: None, or per problem
    None (estimated on the device) or n_t x 3.
    Returns a list of RegistrationResult, each identical to the same problem run alone."""
    from . import lib
    srcs = [_points(s, "source") for s in sources]
    dsts = [_points(t, "target") for t in targets]
    b = len(srcs)
    if len(dsts) != b:
        raise ValueError("sources and targets differ in length (%d vs %d)" % (b, len(dsts)))
    ests = estimation_methods if isinstance(estimation_methods, (list, tuple)) else [estimation_methods] * b
    if len(ests) != b:
        raise ValueError("estimation_methods: one per problem or one for all")
    methods = ests
    ests = [_estimation(m) for m in ests]
    plane = any(m[0] == 1 for m in ests)
    colored = any(m[0] == 3 for m in ests)
    normals = [None] * b
    searches = [None] * b  # a search-parameter object in place of normals: they are estimated on the device
    if plane:
        if target_normals is None or len(target_normals) != b:
            raise ValueError("point-to-plane needs target_normals: one entry per problem")
        for k in range(b):
            if ests[k][0] != 1:
                continue
            if target_normals[k] is None:
                raise ValueError("point-to-plane needs target_normals (problem %d)" % k)
            if isinstance(target_normals[k], _NormalSearch):
                searches[k] = target_normals[k]
                continue
            nv = _points(target_normals[k], "target_normals")
            if nv.shape != dsts[k].shape:
                raise ValueError("target_normals must have the target's shape %s, got %s (problem %d)"
                                 % (dsts[k].shape, nv.shape, k))
            normals[k] = nv
    if colored:
        if target_normals is None or len(target_normals) != b:
            raise ValueError("Colored ICP needs target_normals: one entry per problem")
        for k in range(b):
            if ests[k][0] != 3:
                continue
            if target_normals[k] is None or isinstance(target_normals[k], _NormalSearch):
                raise ValueError("Colored ICP needs target_normals as an array: estimate_normals first "
                                 "(problem %d)" % k)
            nv = _points(target_normals[k], "target_normals")
            if nv.shape != dsts[k].shape:
                raise ValueError("target_normals must have the target's shape %s, got %s (problem %d)"
                                 % (dsts[k].shape, nv.shape, k))
            normals[k] = nv
        if any(sp_ is not None for sp_ in searches):
            raise ValueError("a batch with a Colored-ICP problem takes every target_normals as an array")
    col_s = _per_problem_rows(source_colors, ests, srcs, "source_colors")
    col_t = _per_problem_rows(target_colors, ests, dsts, "target_colors")
    grad_t = _per_problem_rows(target_color_gradients, ests, dsts, "target_color_gradients", required=False)
    gicp = any(m[0] == 2 for m in ests)
    cov_s = _per_problem_covariances(source_covariances, ests, srcs, "source_covariances")
    cov_t = _per_problem_covariances(target_covariances, ests, dsts, "target_covariances")
    rs = np.broadcast_to(np.asarray(max_correspondence_distance, dtype=np.float64), (b,))
    crit = criteria if isinstance(criteria, (list, tuple)) else [criteria] * b
    if len(crit) != b:
        raise ValueError("criteria: one per problem or one for all")
    params = (IcpParamsC * max(b, 1))(*[_params(rs[k], crit[k]) for k in range(b)])
    if inits is None:
        init = None
    else:
        a = np.asarray(inits, dtype=np.float64)
        init = np.ascontiguousarray(np.broadcast_to(a, (b, 4, 4)) if a.shape == (4, 4) else a)
        if init.shape != (b, 4, 4):
            raise ValueError("inits: one 4 x 4 for all problems or b x 4 x 4")
    L = lib()
    n_s = np.array([len(s) for s in srcs], dtype=np.int32)
    n_t = np.array([len(t) for t in dsts], dtype=np.int32)
    sp = (_dp * max(b, 1))(*[s.ctypes.data_as(_dp) for s in srcs])
    tp = (_dp * max(b, 1))(*[t.ctypes.data_as(_dp) for t in dsts])
    corr = [np.zeros((max(int(n), 1), 2), dtype=np.int32) for n in n_s]
    cp = (_ip * max(b, 1))(*[c.ctypes.data_as(_ip) for c in corr])
    out = (IcpResultC * max(b, 1))()
    fn = L.teaser_hip_icp_batch  # point-to-point only: the original entry point
    args = (b, sp, n_s.ctypes.data_as(_ip), tp, n_t.ctypes.data_as(_ip),
            None if init is None else init.ctypes.data_as(_dp), params, out, cp)
    if plane or gicp or colored:
        fn = L.teaser_hip_icp_batch_ex
        args += ((_dp * max(b, 1))(*[None if nv is None else nv.ctypes.data_as(_dp) for nv in normals]),
                 (IcpEstimationC * max(b, 1))(*[IcpEstimationC(*m) for m in ests]))
    if gicp or colored:  # the entry that takes covariances; it serves the other two methods of a mixed batch too
        fn = L.teaser_hip_icp_batch_cov
        args += ((_dp * max(b, 1))(*[None if c is None else c.ctypes.data_as(_dp) for c in cov_s]),
                 (_dp * max(b, 1))(*[None if c is None else c.ctypes.data_as(_dp) for c in cov_t]))
    if colored:  # the entry that takes colours; it serves the other three methods of a mixed batch too
        def ptrs(arrs):
            return (_dp * max(b, 1))(*[None if a is None else a.ctypes.data_as(_dp) for a in arrs])

        fn = L.teaser_hip_icp_batch_color
        args += (ptrs(col_s), ptrs(col_t), ptrs(grad_t),
                 (IcpColorC * max(b, 1))(*[m.record() if isinstance(m, TransformationEstimationForColoredICP)
                                           else IcpColorC(0.968, 0.0, 30, 0) for m in methods]))
    if any(sp_ is not None for sp_ in searches):  # the entry that estimates missing target normals itself
        if not gicp:
            args += (None, None)
        fn = L.teaser_hip_icp_batch_auto
        args += ((IcpNormalSearchC * max(b, 1))(*[IcpNormalSearchC() if sp_ is None else sp_.record()
                                                   for sp_ in searches]),)
    _handle(device).call(fn, *args)
    res = []
    for k in range(b):
        o = out[k]
        res.append(RegistrationResult(np.array(o.transformation[:], dtype=np.float64).reshape(4, 4),
                                      float(o.fitness), float(o.inlier_rmse),
                                      corr[k][:o.n_correspondences].copy(), int(o.iterations)))
    return res


def registration_icp(source, target, max_correspondence_distance, init=np.eye(4), estimation_method=None,
                     criteria=None, device=-1, *, target_normals=None, source_covariances=None,
                     target_covariances=None, source_colors=None, target_colors=None, target_color_gradients=None):
    """Open3D's registration_icp (same argument order): refines `init` so that it maps source onto target.
    source / target: n x 3 points (np.asarray(pcd.points)).  estimation_method: None or
    TransformationEstimationPointToPoint() (with_scaling=False), or TransformationEstimationPointToPlane(kernel), which
    needs target_normals (n_t x 3, np.asarray(target_pcd.normals), or a KDTreeSearchParamHybrid / KDTreeSearchParamKNN
    object to estimate them from the target on the device), or TransformationEstimationForGeneralizedICP(),
    which needs source_covariances (n_s x 3 x 3) and target_covariances (n_t x 3 x 3), or
    TransformationEstimationForColoredICP(), which needs source_colors (n_s x 3), target_colors (n_t x 3) and
    target_normals (n_t x 3) and takes target_color_gradients (n_t x 3; None: estimated on the device)."""
    if estimation_method is not None and not isinstance(
            estimation_method, (TransformationEstimationPointToPoint, TransformationEstimationPointToPlane,
                                TransformationEstimationForGeneralizedICP, TransformationEstimationForColoredICP)):
        raise ValueError("only TransformationEstimationPointToPoint(with_scaling=False), "
                         "TransformationEstimationPointToPlane(kernel), "
                         "TransformationEstimationForGeneralizedICP() and "
                         "TransformationEstimationForColoredICP() are supported")
    if isinstance(estimation_method, TransformationEstimationForColoredICP):
        for given, what in ((source_colors, "source_colors"), (target_colors, "target_colors"),
                            (target_normals, "target_normals")):
            if given is None:
                raise ValueError("TransformationEstimationForColoredICP needs %s" % what)
    if isinstance(estimation_method, TransformationEstimationPointToPlane) and target_normals is None:
        raise ValueError("TransformationEstimationPointToPlane needs target_normals")
    if isinstance(estimation_method, TransformationEstimationForGeneralizedICP):
        if source_covariances is None:
            raise ValueError("TransformationEstimationForGeneralizedICP needs source_covariances")
        if target_covariances is None:
            raise ValueError("TransformationEstimationForGeneralizedICP needs target_covariances")
    return registration_icp_batch([source], [target], max_correspondence_distance, inits=_init(init)[None],
                                  criteria=[criteria], device=device, estimation_methods=[estimation_method],
                                  target_normals=None if target_normals is None else [target_normals],
                                  source_covariances=None if source_covariances is None else [source_covariances],
                                  target_covariances=None if target_covariances is None else [target_covariances],
                                  source_colors=None if source_colors is None else [source_colors],
                                  target_colors=None if target_colors is None else [target_colors],
                                  target_color_gradients=(None if target_color_gradients is None
                                                          else [target_color_gradients]))[0]


def evaluate_registration_batch(sources, targets, max_correspondence_distance, transformations=None, device=-1):
    """Open3D's evaluate_registration for many pairs in one launch sequence: the correspondences, fitness and inlier
    RMSE of the given poses, nothing refined (registration_icp_batch with max_iteration = 0).  transformations: None
    (identity), one 4 x 4 for all or one per pair.  Returns a list of RegistrationResult."""
    return registration_icp_batch(sources, targets, max_correspondence_distance, inits=transformations,
                                  criteria=ICPConvergenceCriteria(max_iteration=0), device=device)


def evaluate_registration(source, target, max_correspondence_distance, transformation=np.eye(4), device=-1):
    """Open3D's evaluate_registration (same argument order): how well `transformation` maps source onto target."""
    return evaluate_registration_batch([source], [target], max_correspondence_distance, _init(transformation)[None],
                                       device)[0]


def get_information_matrix_from_point_clouds_batch(sources, targets, max_correspondence_distance, transformations,
                                                   device=-1, return_results=False):
    """The 6 x 6 information matrices of many registered pairs in one launch sequence (include/teaser_hip.h,
    "Information matrices"; Open3D's get_information_matrix_from_point_clouds): per pair SUM G^T G over the
    correspondences of `transformation` within max_correspondence_distance, G = [-[q]x | I] at the matched target
    point q, so entry (5, 5) is the number of correspondences.  max_correspondence_distance: one value for all or one
    per pair; transformations: one 4 x 4 for all or one per pair.  Returns a b x 6 x 6 array, each matrix identical to
    the same pair evaluated alone; with return_results=True also the list of RegistrationResult that
    evaluate_registration_batch gives for the same arguments."""
    from . import lib
    srcs = [_points(s, "source") for s in sources]
    dsts = [_points(t, "target") for t in targets]
    b = len(srcs)
    if len(dsts) != b:
        raise ValueError("sources and targets differ in length (%d vs %d)" % (b, len(dsts)))
    rs = np.ascontiguousarray(np.broadcast_to(np.asarray(max_correspondence_distance, dtype=np.float64), (b,)))
    a = np.asarray(transformations, dtype=np.float64)
    T = np.ascontiguousarray(np.broadcast_to(a, (b, 4, 4)) if a.shape == (4, 4) else a.reshape(-1, 4, 4) if b == 0 else a)
    if T.shape != (b, 4, 4):
        raise ValueError("transformations: one 4 x 4 for all pairs or b x 4 x 4")
    info = np.zeros((b, 6, 6))
    out = (IcpResultC * max(b, 1))()
    corr = [np.zeros((max(len(s), 1), 2), dtype=np.int32) for s in srcs] if return_results else None
    if b:
        n_s = np.array([len(s) for s in srcs], dtype=np.int32)
        n_t = np.array([len(t) for t in dsts], dtype=np.int32)
        sp = (_dp * b)(*[s.ctypes.data_as(_dp) for s in srcs])
        tp = (_dp * b)(*[t.ctypes.data_as(_dp) for t in dsts])
        cp = None if corr is None else (_ip * b)(*[c.ctypes.data_as(_ip) for c in corr])
        _handle(device).call(lib().teaser_hip_icp_information_batch, b, sp, n_s.ctypes.data_as(_ip), tp,
                             n_t.ctypes.data_as(_ip), T.ctypes.data_as(_dp), rs.ctypes.data_as(_dp),
                             info.ctypes.data_as(_dp), out, cp)
    if not return_results:
        return info
    res = [RegistrationResult(np.array(out[k].transformation[:], dtype=np.float64).reshape(4, 4),
                              float(out[k].fitness), float(out[k].inlier_rmse),
                              corr[k][:out[k].n_correspondences].copy(), int(out[k].iterations)) for k in range(b)]
    return info, res


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation, device=-1):
    """Open3D's get_information_matrix_from_point_clouds (same argument order): the 6 x 6 information matrix of one
    registered pair."""
    return get_information_matrix_from_point_clouds_batch([source], [target], max_correspondence_distance,
                                                          _init(transformation)[None], device)[0]


def covariances_from_normals(normals, epsilon=1e-3):
    """C = I - (1 - epsilon) n n^T / (n^T n) per normal (n x 3 -> n x 3 x 3): the covariance Generalized ICP gives a
    point whose surface normal is n (eigenvalue epsilon along n, 1 across).  A zero or non-finite normal gives the
    identity.  Host arithmetic; lets a caller reuse FPFHEstimation.getNormals()."""
    epsilon = float(epsilon)
    if not (np.isfinite(epsilon) and epsilon > 0):
        raise ValueError("epsilon must be finite and > 0")
    nv = _points(normals, "normals")
    out = np.tile(np.eye(3), (len(nv), 1, 1))
    with np.errstate(all="ignore"):
        nn = (nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2]
    ok = np.isfinite(nv).all(axis=1) & np.isfinite(nn) & (nn > 0)
    v = nv[ok]
    out[ok] -= ((1.0 - epsilon) * v)[:, :, None] * v[:, None, :] / nn[ok][:, None, None]
    return out


def estimate_covariances_batch(clouds, radius, max_nn=20, epsilon=1e-3, device=-1):
    """Generalized-ICP covariances of many clouds in one launch sequence (include/teaser_hip.h, "Covariance
    estimation"): per point the max_nn nearest neighbours inside `radius` (the point itself included), their sample
    covariance, and C = I - (1 - epsilon) n n^T with n its smallest eigenvector; the identity below 3 neighbours.
    radius, max_nn, epsilon: one value for all clouds or one per cloud.  Returns a list of n x 3 x 3 arrays, each
    identical to the same cloud estimated alone."""
    from . import lib
    pts = [_points(c, "points") for c in clouds]
    b = len(pts)
    rs = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (b,)))
    es = np.ascontiguousarray(np.broadcast_to(np.asarray(epsilon, dtype=np.float64), (b,)))
    ks = np.ascontiguousarray(np.broadcast_to(np.asarray(max_nn), (b,)).astype(np.int32))
    if b and (ks.min() < 3 or ks.max() > MAX_NN_LIMIT):
        raise ValueError("max_nn must lie in [3, %d]" % MAX_NN_LIMIT)
    if b and not (np.isfinite(rs).all() and (rs > 0).all()):
        raise ValueError("radius must be finite and > 0")
    if b and not (np.isfinite(es).all() and (es > 0).all()):
        raise ValueError("epsilon must be finite and > 0")
    out = [np.empty((len(p), 3, 3)) for p in pts]
    if b == 0:
        return out
    n = np.array([len(p) for p in pts], dtype=np.int32)
    pp = (_dp * b)(*[p.ctypes.data_as(_dp) for p in pts])
    op = (_dp * b)(*[o.ctypes.data_as(_dp) for o in out])
    _handle(device).call(lib().teaser_hip_icp_covariances_batch, b, pp, n.ctypes.data_as(_ip),
                         rs.ctypes.data_as(_dp), ks.ctypes.data_as(_ip), es.ctypes.data_as(_dp), op)
    return out


def estimate_normals_batch(clouds, search_param, towards=None, along=None, covariances=False, eigenvalues=False,
                           device=-1):
    """Normals of many clouds in one launch sequence (include/teaser_hip.h, "Normal estimation"; Open3D's
    estimate_normals).  search_param: a KDTreeSearchParamHybrid or KDTreeSearchParamKNN for all clouds or one per
    cloud; towards / along: None, or a point / direction (for all clouds) the normals are oriented by, overriding the
    search parameter's own orientation.  Returns a list with one entry per cloud: the n x 3 normals, or a tuple
    (normals[, covariances n x 3 x 3 (the raw sample covariances)][, eigenvalues n x 3 ascending]) when asked for.
    Each cloud's result is identical to the same cloud estimated alone."""
    from . import lib
    pts = [_points(c, "points") for c in clouds]
    b = len(pts)
    sps = list(search_param) if isinstance(search_param, (list, tuple)) else [search_param] * b
    if len(sps) != b or not all(isinstance(p, _NormalSearch) for p in sps):
        raise ValueError("search_param: a KDTreeSearchParamHybrid / KDTreeSearchParamKNN, one for all or one per cloud")
    if towards is not None and along is not None:
        raise ValueError("towards and along exclude each other")
    if towards is not None:
        sps = [p.towards(towards) for p in sps]
    if along is not None:
        sps = [p.along(along) for p in sps]
    nrm = [np.empty((len(p), 3)) for p in pts]
    cov = [np.empty((len(p), 3, 3)) for p in pts] if covariances else None
    eig = [np.empty((len(p), 3)) for p in pts] if eigenvalues else None
    if b:
        n = np.array([len(p) for p in pts], dtype=np.int32)
        ptrs = lambda arrs: None if arrs is None else (_dp * b)(*[a.ctypes.data_as(_dp) for a in arrs])  # noqa: E731
        _handle(device).call(lib().teaser_hip_icp_normals_batch, b, ptrs(pts), n.ctypes.data_as(_ip),
                             (IcpNormalSearchC * b)(*[p.record() for p in sps]), ptrs(nrm), ptrs(cov), ptrs(eig))
    if not covariances and not eigenvalues:
        return nrm
    return [tuple(x[k] for x in (nrm, cov, eig) if x is not None) for k in range(b)]


def estimate_normals(points, search_param, towards=None, along=None, covariances=False, eigenvalues=False, device=-1):
    """estimate_normals_batch for one cloud: n x 3 points -> n x 3 unit normals (or the tuple described there)."""
    return estimate_normals_batch([points], search_param, towards, along, covariances, eigenvalues, device)[0]


def surface_variation(eigenvalues):
    """lambda0 / (lambda0 + lambda1 + lambda2) per row of ascending eigenvalues (estimate_normals(...,
    eigenvalues=True)); 0 where the sum is 0."""
    e = np.asarray(eigenvalues, dtype=np.float64)
    s = (e[..., 0] + e[..., 1]) + e[..., 2]
    out = np.zeros(s.shape)
    np.divide(e[..., 0], s, out=out, where=s != 0)
    return out


def estimate_covariances(points, radius, max_nn=20, epsilon=1e-3, device=-1):
    """estimate_covariances_batch for one cloud: n x 3 points -> n x 3 x 3 covariances."""
    return estimate_covariances_batch([points], radius, max_nn, epsilon, device)[0]


def registration_generalized_icp(source, target, max_correspondence_distance, init=np.eye(4), estimation_method=None,
                                 criteria=None, source_covariances=None, target_covariances=None,
                                 search_radius=None, max_nn=20, device=-1):
    """Open3D's registration_generalized_icp (same leading arguments).  Covariances that are not given are estimated on
    the GPU from the cloud itself with estimate_covariances(cloud, search_radius, max_nn, estimation.epsilon); without
    them and without search_radius the call raises ValueError."""
    est = TransformationEstimationForGeneralizedICP() if estimation_method is None else estimation_method
    if not isinstance(est, TransformationEstimationForGeneralizedICP):
        raise ValueError("estimation_method must be TransformationEstimationForGeneralizedICP()")
    missing = [c for c, given in ((source, source_covariances), (target, target_covariances)) if given is None]
    if missing:
        if search_radius is None:
            raise ValueError("registration_generalized_icp needs source_covariances and target_covariances, or a "
                             "search_radius to estimate them with")
        found = iter(estimate_covariances_batch(missing, search_radius, max_nn, est.epsilon, device))
        if source_covariances is None:
            source_covariances = next(found)
        if target_covariances is None:
            target_covariances = next(found)
    return registration_icp(source, target, max_correspondence_distance, init, est, criteria, device,
                            source_covariances=source_covariances, target_covariances=target_covariances)


def estimate_color_gradients_batch(clouds, normals, colors, radius, max_nn=30, device=-1):
    """The colour gradients Colored ICP uses, for many clouds in one launch sequence (include/teaser_hip.h, "ICP
    refinement: Colored ICP"): per point the max_nn nearest neighbours inside `radius`, projected onto the tangent plane
    of its normal, and the least-squares gradient of the intensity ((r + g) + b) / 3 over them; 0 below 4 neighbours.
    clouds, normals, colors: one n x 3 array per cloud each; radius, max_nn: one value for all clouds or one per cloud.
    Returns a list of n x 3 arrays, each identical to the same cloud estimated alone."""
    from . import lib
    pts = [_points(c, "points") for c in clouds]
    b = len(pts)
    if len(normals) != b or len(colors) != b:
        raise ValueError("clouds, normals and colors differ in length")
    nrm = [_points(a, "normals") for a in normals]
    col = [_points(a, "colors") for a in colors]
    for k in range(b):
        if nrm[k].shape != pts[k].shape or col[k].shape != pts[k].shape:
            raise ValueError("normals and colors must have the cloud's shape %s (cloud %d)" % (pts[k].shape, k))
    rs = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (b,)))
    ks = np.ascontiguousarray(np.broadcast_to(np.asarray(max_nn), (b,)).astype(np.int32))
    if b and (ks.min() < 4 or ks.max() > MAX_NN_LIMIT):
        raise ValueError("max_nn must lie in [4, %d]" % MAX_NN_LIMIT)
    if b and not (np.isfinite(rs).all() and (rs > 0).all()):
        raise ValueError("radius must be finite and > 0")
    out = [np.empty((len(p), 3)) for p in pts]
    if b == 0:
        return out
    n = np.array([len(p) for p in pts], dtype=np.int32)
    ptrs = lambda arrs: (_dp * b)(*[a.ctypes.data_as(_dp) for a in arrs])  # noqa: E731
    _handle(device).call(lib().teaser_hip_icp_color_gradients_batch, b, ptrs(pts), n.ctypes.data_as(_ip), ptrs(nrm),
                         ptrs(col), rs.ctypes.data_as(_dp), ks.ctypes.data_as(_ip), ptrs(out))
    return out


def estimate_color_gradients(points, normals, colors, radius, max_nn=30, device=-1):
    """estimate_color_gradients_batch for one cloud: n x 3 points, normals and colours -> n x 3 gradients."""
    return estimate_color_gradients_batch([points], [normals], [colors], radius, max_nn, device)[0]


def registration_colored_icp(source, target, max_correspondence_distance, init=np.eye(4), estimation_method=None,
                             criteria=None, *, source_colors=None, target_colors=None, target_normals=None,
                             gradient_radius=None, gradient_max_nn=30, target_color_gradients=None, device=-1):
    """Open3D's registration_colored_icp (same leading arguments; the colours and normals Open3D reads from its point
    clouds are keyword arguments here).  estimation_method: None or TransformationEstimationForColoredICP(...);
    gradient_radius / gradient_max_nn: the neighbourhood of the target's colour gradients (None: twice
    max_correspondence_distance, Open3D's choice), unless target_color_gradients gives them.  The target normals are not
    estimated here: estimate_normals first."""
    est = TransformationEstimationForColoredICP() if estimation_method is None else estimation_method
    if not isinstance(est, TransformationEstimationForColoredICP):
        raise ValueError("estimation_method must be TransformationEstimationForColoredICP()")
    for given, what in ((source_colors, "source_colors"), (target_colors, "target_colors"),
                        (target_normals, "target_normals")):
        if given is None:
            raise ValueError("registration_colored_icp needs %s" % what)
    est = TransformationEstimationForColoredICP(
        est.lambda_geometric, est.kernel, est.gradient_radius if gradient_radius is None else gradient_radius,
        est.gradient_max_nn if gradient_max_nn == 30 else gradient_max_nn)
    return registration_icp(source, target, max_correspondence_distance, init, est, criteria, device,
                            target_normals=target_normals, source_colors=source_colors, target_colors=target_colors,
                            target_color_gradients=target_color_gradients)
