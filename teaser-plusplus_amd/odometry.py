"""RGB-D odometry on the GPU with the surface of open3d.pipelines.odometry: the motion between two RGB-D frames and its
information matrix, the first stage of Open3D's reconstruction pipeline (make_fragments).

    source = RGBDImage.create_from_color_and_depth(color0, depth0)
    target = RGBDImage.create_from_color_and_depth(color1, depth1)
    success, trans, info = compute_rgbd_odometry(source, target, intrinsic)        # source -> target, 4 x 4, 6 x 6
    results = compute_rgbd_odometry_batch(sources, targets, intrinsic)             # every pair in ONE launch sequence

``trans`` and ``info`` are what PoseGraphEdge and UniformTSDFVolume.integrate take.  A single pair is bound by its about
hundred small launches; a batch shares them, and every pair's result is identical to the pair run alone.  The arithmetic
is written out in include/teaser_hip.h ("RGB-D odometry"): float32 images as Open3D forms them, FP64 from the
correspondences on, every sum in a stated order, the sine and cosine of the pose update from plain arithmetic; bit parity
with an Open3D binary is not claimed.

Images are numpy arrays: depth ``height x width`` uint16 or float32, colour ``height x width x 3`` uint8 or ``height x
width`` float32 (an intensity).  The conversion to float32 metres and to intensity happens on the device.  Rows may lie
any distance apart.  Source and target of a pair must agree in size and dtypes.  The calls run on the ICP handle of the
device.  Without a GPU they raise TeaserHipError (NO_DEVICE): there is no CPU path."""
import ctypes as C
import math

import numpy as np

from .icp import _handle
from .rgbd import _each, _fxfycxcy, _image, _is_intrinsic, _is_matrix

_vp = C.c_void_p
MAX_LEVELS = 8
PLANES = ("I_s", "I_t", "D_s", "D_t", "X", "Y", "Z", "I_t_dx", "I_t_dy", "D_t_dx", "D_t_dy")


class OdometryOptionC(C.Structure):
    """teaser_icp_odometry_option_c (include/teaser_hip.h)."""
    _fields_ = [("n_levels", C.c_int32), ("iterations", C.c_int32 * 8), ("reserved", C.c_int32 * 3),
                ("depth_diff_max", C.c_double), ("depth_min", C.c_double), ("depth_max", C.c_double),
                ("reserved2", C.c_double)]


class OdometryPairC(C.Structure):
    """teaser_icp_odometry_pair_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("target_width", C.c_int32), ("target_height", C.c_int32),
                ("depth_format", C.c_int32), ("color_format", C.c_int32), ("jacobian", C.c_int32), ("reserved", C.c_int32),
                ("source_depth_row_bytes", C.c_int64), ("source_color_row_bytes", C.c_int64),
                ("target_depth_row_bytes", C.c_int64), ("target_color_row_bytes", C.c_int64), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("odo_init", C.c_double * 16),
                ("depth_scale", C.c_double), ("depth_trunc", C.c_double)]


class OdometryResultC(C.Structure):
    """teaser_icp_odometry_result_c (include/teaser_hip.h)."""
    _fields_ = [("success", C.c_int32), ("count", C.c_int32), ("iterations", C.c_int32), ("reserved", C.c_int32),
                ("transformation", C.c_double * 16), ("information", C.c_double * 36)]


class OdometryTraceC(C.Structure):
    """teaser_icp_odometry_trace_c (include/teaser_hip.h)."""
    _fields_ = [("level", C.c_int32), ("executed", C.c_int32), ("count", C.c_int32), ("failed", C.c_int32),
                ("e", C.c_double), ("A", C.c_double * 21), ("g", C.c_double * 6), ("pose", C.c_double * 16),
                ("reserved", C.c_double * 2)]


assert (C.sizeof(OdometryOptionC), C.sizeof(OdometryPairC), C.sizeof(OdometryResultC), C.sizeof(OdometryTraceC)) == \
    (80, 240, 432, 384)  # the header asserts the same


def declare(L):
    """ctypes signatures of the entry points (called by the package's lib())."""
    pp = C.POINTER(_vp)
    L.teaser_hip_icp_odometry_option_default.argtypes = [C.POINTER(OdometryOptionC)]
    L.teaser_hip_icp_rgbd_odometry_batch.argtypes = [_vp, C.c_int32, C.POINTER(OdometryPairC), C.POINTER(OdometryOptionC),
                                                     pp, pp, pp, pp, C.POINTER(OdometryResultC), pp]
    L.teaser_hip_icp_rgbd_odometry_pyramid_batch.argtypes = [_vp, C.c_int32, C.POINTER(OdometryPairC),
                                                             C.POINTER(OdometryOptionC), pp, pp, pp, pp, pp]


class RGBDOdometryJacobianFromColorTerm:
    """Open3D's RGBDOdometryJacobianFromColorTerm: the photometric row alone."""
    kind = 0


class RGBDOdometryJacobianFromHybridTerm:
    """Open3D's RGBDOdometryJacobianFromHybridTerm: the photometric and the geometric row (lambda = 0.968)."""
    kind = 1


class OdometryOption:
    """Open3D's OdometryOption.  iteration_number_per_pyramid_level: the FIRST entry belongs to the COARSEST level;
    max_depth_diff is accepted as another name of depth_diff_max (Open3D has used both)."""

    def __init__(self, iteration_number_per_pyramid_level=(20, 10, 5), depth_diff_max=0.03, depth_min=0.0, depth_max=4.0,
                 max_depth_diff=None):
        self.iteration_number_per_pyramid_level = list(iteration_number_per_pyramid_level)
        self.depth_diff_max = depth_diff_max if max_depth_diff is None else max_depth_diff
        self.depth_min, self.depth_max = depth_min, depth_max

    @property
    def max_depth_diff(self):
        return self.depth_diff_max

    @max_depth_diff.setter
    def max_depth_diff(self, v):
        self.depth_diff_max = v

    def _record(self):
        it = list(self.iteration_number_per_pyramid_level)
        if not 1 <= len(it) <= MAX_LEVELS:
            raise ValueError("iteration_number_per_pyramid_level must have 1 to 8 entries")
        if any(int(v) != v or v < 0 for v in it):
            raise ValueError("iteration_number_per_pyramid_level must hold integers >= 0")
        for name in ("depth_diff_max", "depth_min", "depth_max"):
            v = float(getattr(self, name))
            if not math.isfinite(v) or (name != "depth_max" and v < 0):
                raise ValueError("%s must be finite%s" % (name, "" if name == "depth_max" else " and >= 0"))
        rec = OdometryOptionC()
        rec.n_levels = len(it)
        for k, v in enumerate(it):
            rec.iterations[k] = int(v)
        rec.depth_diff_max, rec.depth_min, rec.depth_max = float(self.depth_diff_max), float(self.depth_min), float(self.depth_max)
        return rec

    def __repr__(self):
        return "OdometryOption(iteration_number_per_pyramid_level=%r, depth_diff_max=%r, depth_min=%r, depth_max=%r)" % (
            self.iteration_number_per_pyramid_level, self.depth_diff_max, self.depth_min, self.depth_max)


class RGBDImage:
    """Open3D's geometry.RGBDImage as this package needs it: the two arrays and the parameters of their conversion,
    which happens on the device."""

    def __init__(self, color, depth, depth_scale=1000.0, depth_trunc=3.0):
        self.color, self.depth = color, depth
        self.depth_scale, self.depth_trunc = float(depth_scale), float(depth_trunc)

    @staticmethod
    def create_from_color_and_depth(color, depth, depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True):
        if not convert_rgb_to_intensity:
            raise ValueError("convert_rgb_to_intensity must be True: odometry works on the intensity")
        return RGBDImage(color, depth, depth_scale, depth_trunc)


class OdometryTrace:
    """One pair's iterations in execution order, as arrays with one row per iteration: level, executed, count, failed,
    e (the sum of squared residuals), A (21: J^T J by rows), g (6: J^T r) and pose (4 x 4 after the update)."""

    def __init__(self, records):
        n = len(records)
        a = np.frombuffer(records, dtype=np.uint8).reshape(n, C.sizeof(OdometryTraceC)) if n else np.zeros((0, 384), np.uint8)
        ints = a[:, :16].copy().view(np.int32).reshape(n, 4)
        dbl = a[:, 16:].copy().view(np.float64).reshape(n, 46)
        self.level, self.executed, self.count, self.failed = ints[:, 0], ints[:, 1], ints[:, 2], ints[:, 3]
        self.e, self.A, self.g, self.pose = dbl[:, 0], dbl[:, 1:22], dbl[:, 22:28], dbl[:, 28:44].reshape(n, 4, 4)

    def __len__(self):
        return len(self.level)


class OdometryResult:
    """One pair: success, transformation (4 x 4, source to target), information (6 x 6), count (the correspondences at
    the final pose), iterations (executed) and, where asked for, trace.  Unpacks like Open3D's return value:
    ``success, trans, info = result``."""

    def __init__(self, success, transformation, information, count, iterations, trace=None):
        self.success, self.transformation, self.information = success, transformation, information
        self.count, self.iterations, self.trace = count, iterations, trace

    def __iter__(self):
        return iter((self.success, self.transformation, self.information))


def _pairs(sources, targets, intrinsic, odo_init, jacobian, option):
    """The checks of a call and its records: (b, pair records, option record, the four pointer arrays, what to keep
    alive)."""
    if not isinstance(option, OdometryOption):
        raise ValueError("option must be an OdometryOption")
    opt = option._record()
    sources, targets = list(sources), list(targets)
    b = len(sources)
    if len(targets) != b:
        raise ValueError("targets: one RGBDImage per source")
    K = [_fxfycxcy(k) for k in _each(intrinsic, b, "intrinsic", _is_intrinsic)]
    init = _each(odo_init, b, "odo_init", _is_matrix)
    jac = _each(jacobian, b, "jacobian", lambda v: not isinstance(v, (list, tuple)))
    recs = (OdometryPairC * max(b, 1))()
    keep, ptrs = [], [(_vp * max(b, 1))() for _ in range(4)]
    for k in range(b):
        s, t = sources[k], targets[k]
        if not isinstance(s, RGBDImage) or not isinstance(t, RGBDImage):
            raise ValueError("source and target must be RGBDImage objects (pair %d)" % k)
        if (s.depth_scale, s.depth_trunc) != (t.depth_scale, t.depth_trunc):
            raise ValueError("source and target differ in depth_scale or depth_trunc (pair %d)" % k)
        imgs = []
        for img, what in ((s, "source"), (t, "target")):
            d, dpx = _image(img.depth, what + " depth", (np.uint16, np.float32), (1,))
            if d.ndim != 2:
                raise ValueError("%s depth has shape %s" % (what, d.shape))
            c, cpx = _image(img.color, what + " color", (np.uint8, np.float32), (1, 3))
            if (c.dtype == np.uint8) != (c.ndim == 3):
                raise ValueError("%s color must be uint8 x 3 or a float32 intensity, got %s of shape %s" % (what, c.dtype, c.shape))
            if c.shape[:2] != d.shape:
                raise ValueError("%s color has shape %s beside a depth image of shape %s" % (what, c.shape, d.shape))
            imgs += [(d, dpx), (c, cpx)]
        (sd, _), (sc, _), (td, _), (tc, _) = imgs
        if sd.shape != td.shape:
            raise ValueError("source and target differ in size: %s and %s (pair %d)" % (sd.shape, td.shape, k))
        if sd.dtype != td.dtype or sc.dtype != tc.dtype:
            raise ValueError("source and target differ in dtype (pair %d)" % k)
        h, w = sd.shape
        if min(h, w) >> (opt.n_levels - 1) < 1:
            raise ValueError("an image of %d x %d has no pixel at pyramid level %d (pair %d)" % (w, h, opt.n_levels - 1, k))
        fx, fy, cx, cy = K[k]
        if not (math.isfinite(fx) and math.isfinite(fy) and fx > 0 and fy > 0 and math.isfinite(cx) and math.isfinite(cy)):
            raise ValueError("intrinsic: fx and fy must be finite and > 0, cx and cy finite (pair %d)" % k)
        T = np.array(np.eye(4) if init[k] is None else init[k], dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise ValueError("odo_init must be a finite 4 x 4 matrix (pair %d)" % k)
        kind = getattr(jac[k], "kind", jac[k])
        if kind not in (0, 1):
            raise ValueError("jacobian must be RGBDOdometryJacobianFromColorTerm or RGBDOdometryJacobianFromHybridTerm")
        if not (math.isfinite(s.depth_scale) and s.depth_scale > 0 and math.isfinite(s.depth_trunc)):
            raise ValueError("depth_scale must be finite and > 0, depth_trunc finite (pair %d)" % k)
        r = recs[k]
        r.width = r.target_width = w
        r.height = r.target_height = h
        r.depth_format, r.color_format, r.jacobian = (0 if sd.dtype == np.uint16 else 1), (1 if sc.dtype == np.uint8 else 2), kind
        for name, (a, px) in zip(("source_depth", "source_color", "target_depth", "target_color"), imgs):
            setattr(r, name + "_row_bytes", a.strides[0] if a.size else a.shape[1] * px)
        r.fx, r.fy, r.cx, r.cy = fx, fy, cx, cy
        r.odo_init[:] = list(T.ravel())
        r.depth_scale, r.depth_trunc = s.depth_scale, s.depth_trunc
        for p, (a, _) in zip(ptrs, imgs):
            p[k] = a.ctypes.data_as(_vp)
            keep.append(a)
    return b, recs, opt, ptrs, keep


def compute_rgbd_odometry_batch(sources, targets, intrinsic, odo_init=None, jacobian=RGBDOdometryJacobianFromHybridTerm,
                                option=None, return_trace=False, device=-1):
    """Per pair an OdometryResult, all pairs in one launch sequence (include/teaser_hip.h, "RGB-D odometry").  sources,
    targets: lists of RGBDImage; intrinsic, odo_init, jacobian: one for all pairs or a list with one per pair."""
    from . import lib
    b, recs, opt, ptrs, keep = _pairs(sources, targets, intrinsic, odo_init, jacobian, OdometryOption() if option is None else option)
    if b == 0:
        return []
    n_iter = sum(opt.iterations[k] for k in range(opt.n_levels))
    res = (OdometryResultC * b)()
    traces = [(OdometryTraceC * max(n_iter, 1))() for _ in range(b)] if return_trace else None
    tp = (_vp * b)(*[C.cast(t, _vp) for t in traces]) if return_trace else None
    _handle(device).call(lib().teaser_hip_icp_rgbd_odometry_batch, b, recs, C.byref(opt), *ptrs, res, tp)
    out = []
    for k in range(b):
        r = res[k]
        tr = OdometryTrace((OdometryTraceC * n_iter).from_buffer(traces[k]) if n_iter else b"") if return_trace else None
        out.append(OdometryResult(bool(r.success), np.array(r.transformation[:]).reshape(4, 4),
                                  np.array(r.information[:]).reshape(6, 6), int(r.count), int(r.iterations), tr))
    return out


def compute_rgbd_odometry(source, target, intrinsic, odo_init=None, jacobian=RGBDOdometryJacobianFromHybridTerm,
                          option=None, device=-1):
    """Open3D's compute_rgbd_odometry(source, target, pinhole_camera_intrinsic, odo_init, jacobian, option):
    (success, 4 x 4 transformation, 6 x 6 information)."""
    r = compute_rgbd_odometry_batch([source], [target], intrinsic, odo_init, jacobian, option, device=device)[0]
    return r.success, r.transformation, r.information


def rgbd_odometry_pyramid_batch(sources, targets, intrinsic, odo_init=None, option=None, device=-1):
    """The preprocessing and pyramid stage alone, by the kernels the odometry runs: per pair a list of levels, each a dict
    of float32 images named I_s, I_t, D_s, D_t, XYZ (height x width x 3), I_t_dx, I_t_dy, D_t_dx, D_t_dy."""
    from . import lib
    b, recs, opt, ptrs, keep = _pairs(sources, targets, intrinsic, odo_init, RGBDOdometryJacobianFromHybridTerm,
                                      OdometryOption() if option is None else option)
    if b == 0:
        return []
    L = opt.n_levels
    dims = [[(recs[k].height >> l, recs[k].width >> l) for l in range(L)] for k in range(b)]
    flat = [np.empty(len(PLANES) * sum(h * w for h, w in dims[k]), dtype=np.float32) for k in range(b)]
    out_ptrs = (_vp * b)(*[a.ctypes.data_as(_vp) for a in flat])
    _handle(device).call(lib().teaser_hip_icp_rgbd_odometry_pyramid_batch, b, recs, C.byref(opt), *ptrs, out_ptrs)
    out = []
    for k in range(b):
        at, levels = 0, []
        for h, w in dims[k]:
            planes = {name: flat[k][at + i * h * w: at + (i + 1) * h * w].reshape(h, w) for i, name in enumerate(PLANES)}
            lev = {n: planes[n] for n in PLANES if n not in "XYZ"}
            lev["XYZ"] = np.stack([planes["X"], planes["Y"], planes["Z"]], axis=2)
            levels.append(lev)
            at += len(PLANES) * h * w
        out.append(levels)
    return out


# ---- depth odometry (include/teaser_hip.h, "Depth odometry") -----------------------------------------------------------
DEPTH_PLANES = ("D_s", "D_t", "Vs_x", "Vs_y", "Vs_z", "Vt_x", "Vt_y", "Vt_z", "Nt_x", "Nt_y", "Nt_z")


class DepthOdometryOptionC(C.Structure):
    """teaser_icp_depth_odometry_option_c (include/teaser_hip.h)."""
    _fields_ = [("n_levels", C.c_int32), ("iterations", C.c_int32 * 8), ("reserved", C.c_int32 * 3),
                ("depth_outlier_trunc", C.c_double), ("depth_huber_delta", C.c_double), ("depth_min", C.c_double),
                ("depth_max", C.c_double), ("relative_rmse", C.c_double), ("relative_fitness", C.c_double),
                ("reserved2", C.c_double * 2)]


class DepthOdometryPairC(C.Structure):
    """teaser_icp_depth_odometry_pair_c (include/teaser_hip.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth_format", C.c_int32), ("reserved", C.c_int32),
                ("source_depth_row_bytes", C.c_int64), ("target_depth_row_bytes", C.c_int64), ("fx", C.c_double),
                ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("init", C.c_double * 16),
                ("depth_scale", C.c_double), ("reserved2", C.c_double)]


class DepthOdometryResultC(C.Structure):
    """teaser_icp_depth_odometry_result_c (include/teaser_hip.h)."""
    _fields_ = [("success", C.c_int32), ("count", C.c_int32), ("iterations", C.c_int32), ("converged_levels", C.c_int32),
                ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("transformation", C.c_double * 16),
                ("information", C.c_double * 36)]


class DepthOdometryTraceC(C.Structure):
    """teaser_icp_depth_odometry_trace_c (include/teaser_hip.h)."""
    _fields_ = [("level", C.c_int32), ("executed", C.c_int32), ("count", C.c_int32), ("failed", C.c_int32),
                ("converged", C.c_int32), ("reserved", C.c_int32), ("e", C.c_double), ("A", C.c_double * 21),
                ("g", C.c_double * 6), ("pose", C.c_double * 16), ("reserved2", C.c_double)]


assert (C.sizeof(DepthOdometryOptionC), C.sizeof(DepthOdometryPairC), C.sizeof(DepthOdometryResultC),
        C.sizeof(DepthOdometryTraceC)) == (112, 208, 448, 384)  # the header asserts the same


def declare_depth(L):
    """ctypes signatures of the depth odometry entry points (called by the package's lib())."""
    pp = C.POINTER(_vp)
    L.teaser_hip_icp_depth_odometry_option_default.argtypes = [C.POINTER(DepthOdometryOptionC)]
    L.teaser_hip_icp_depth_odometry_pairs.argtypes = [_vp, C.c_int32, C.POINTER(DepthOdometryPairC),
                                                      C.POINTER(DepthOdometryOptionC), pp, pp,
                                                      C.POINTER(DepthOdometryResultC), pp]
    L.teaser_hip_icp_depth_odometry_pyramid_pairs.argtypes = [_vp, C.c_int32, C.POINTER(DepthOdometryPairC),
                                                              C.POINTER(DepthOdometryOptionC), pp, pp, pp]


class OdometryConvergenceCriteria:
    """Open3D's t.pipelines.odometry.OdometryConvergenceCriteria: the largest number of iterations of one level and the
    two relative thresholds behind which the level stops."""

    def __init__(self, max_iteration, relative_rmse=1e-6, relative_fitness=1e-6):
        self.max_iteration, self.relative_rmse, self.relative_fitness = max_iteration, relative_rmse, relative_fitness

    def __repr__(self):
        return "OdometryConvergenceCriteria(max_iteration=%r, relative_rmse=%r, relative_fitness=%r)" % (
            self.max_iteration, self.relative_rmse, self.relative_fitness)


class OdometryLossParams:
    """Open3D's t.pipelines.odometry.OdometryLossParams as depth odometry reads it: depth_outlier_trunc (the largest
    point-to-plane residual of a correspondence, metres) and depth_huber_delta."""

    def __init__(self, depth_outlier_trunc=0.07, depth_huber_delta=0.05):
        self.depth_outlier_trunc, self.depth_huber_delta = depth_outlier_trunc, depth_huber_delta


class DepthOdometryOption:
    """The options of depth odometry.  criteria: one OdometryConvergenceCriteria (or a plain iteration count) per level,
    the FIRST entry belonging to the COARSEST level; the relative thresholds of the call are those of the first entry,
    and all entries must agree on them.  loss: OdometryLossParams.  depth_scale divides uint16 depth; float32 depth is
    taken as metres.  depth_min / depth_max: samples outside (depth_min, depth_max] are invalid."""

    def __init__(self, criteria=(10, 5, 3), loss=None, depth_scale=1000.0, depth_min=0.0, depth_max=3.0):
        self.criteria = list(criteria)
        self.loss = OdometryLossParams() if loss is None else loss
        self.depth_scale, self.depth_min, self.depth_max = depth_scale, depth_min, depth_max

    def _record(self):
        crit = [c if isinstance(c, OdometryConvergenceCriteria) else OdometryConvergenceCriteria(c) for c in self.criteria]
        if not 1 <= len(crit) <= MAX_LEVELS:
            raise ValueError("criteria must have 1 to 8 entries")
        if any(int(c.max_iteration) != c.max_iteration or c.max_iteration < 0 for c in crit):
            raise ValueError("criteria: max_iteration must be an integer >= 0")
        if any((c.relative_rmse, c.relative_fitness) != (crit[0].relative_rmse, crit[0].relative_fitness) for c in crit):
            raise ValueError("criteria: every level must have the same relative_rmse and relative_fitness")
        if not isinstance(self.loss, OdometryLossParams):
            raise ValueError("loss must be an OdometryLossParams")
        rec = DepthOdometryOptionC()
        rec.n_levels = len(crit)
        for k, c in enumerate(crit):
            rec.iterations[k] = int(c.max_iteration)
        for name, v in (("relative_rmse", crit[0].relative_rmse), ("relative_fitness", crit[0].relative_fitness)):
            if not math.isfinite(float(v)):
                raise ValueError("%s must be finite" % name)
            setattr(rec, name, float(v))
        for name in ("depth_outlier_trunc", "depth_huber_delta"):
            v = float(getattr(self.loss, name))
            if not (math.isfinite(v) and v > 0):
                raise ValueError("%s must be finite and > 0" % name)
            setattr(rec, name, v)
        for name in ("depth_min", "depth_max"):
            v = float(getattr(self, name))
            if not math.isfinite(v) or (name == "depth_min" and v < 0):
                raise ValueError("%s must be finite%s" % (name, " and >= 0" if name == "depth_min" else ""))
            setattr(rec, name, v)
        if not (math.isfinite(float(self.depth_scale)) and float(self.depth_scale) > 0):
            raise ValueError("depth_scale must be finite and > 0")
        return rec


class DepthOdometryTrace:
    """One pair's iterations in launch order, as arrays with one row per iteration: level, executed, count, failed,
    converged, e (the sum of the Huber terms), A (21: J^T J by rows), g (6) and pose (4 x 4 after the update)."""

    def __init__(self, records):
        n = len(records)
        a = np.frombuffer(records, dtype=np.uint8).reshape(n, C.sizeof(DepthOdometryTraceC)) if n else np.zeros((0, 384), np.uint8)
        ints = a[:, :24].copy().view(np.int32).reshape(n, 6)
        dbl = a[:, 24:].copy().view(np.float64).reshape(n, 45)
        self.level, self.executed, self.count, self.failed, self.converged = (ints[:, k] for k in range(5))
        self.e, self.A, self.g, self.pose = dbl[:, 0], dbl[:, 1:22], dbl[:, 22:28], dbl[:, 28:44].reshape(n, 4, 4)

    def __len__(self):
        return len(self.level)


class DepthOdometryResult:
    """One pair: success, transformation (4 x 4, source to target), information (6 x 6), fitness and inlier_rmse (of the
    last executed iteration), count, iterations (executed), converged_levels (bit l: level l converged) and, where
    asked for, trace.  Unpacks as ``success, transformation, information, fitness, inlier_rmse = result``."""

    def __init__(self, success, transformation, information, fitness, inlier_rmse, count, iterations, converged_levels,
                 trace=None):
        self.success, self.transformation, self.information = success, transformation, information
        self.fitness, self.inlier_rmse, self.count, self.iterations = fitness, inlier_rmse, count, iterations
        self.converged_levels, self.trace = converged_levels, trace

    def __iter__(self):
        return iter((self.success, self.transformation, self.information, self.fitness, self.inlier_rmse))


def _depth_pairs(sources, targets, intrinsic, init, option):
    """The checks of a depth odometry call and its records: (b, pair records, option record, the two pointer arrays,
    what to keep alive)."""
    if not isinstance(option, DepthOdometryOption):
        raise ValueError("option must be a DepthOdometryOption")
    opt = option._record()
    sources, targets = list(sources), list(targets)
    b = len(sources)
    if len(targets) != b:
        raise ValueError("targets: one depth image per source")
    K = [_fxfycxcy(k) for k in _each(intrinsic, b, "intrinsic", _is_intrinsic)]
    inits = _each(init, b, "init", _is_matrix)
    recs = (DepthOdometryPairC * max(b, 1))()
    keep, ptrs = [], [(_vp * max(b, 1))() for _ in range(2)]
    for k in range(b):
        imgs = []
        for img, what in ((sources[k], "source"), (targets[k], "target")):
            d, dpx = _image(img, what + " depth", (np.uint16, np.float32), (1,))
            if d.ndim != 2:
                raise ValueError("%s depth has shape %s" % (what, d.shape))
            imgs.append((d, dpx))
        (sd, _), (td, _) = imgs
        if sd.shape != td.shape:
            raise ValueError("source and target differ in size: %s and %s (pair %d)" % (sd.shape, td.shape, k))
        if sd.dtype != td.dtype:
            raise ValueError("source and target differ in dtype (pair %d)" % k)
        h, w = sd.shape
        if min(h, w) >> (opt.n_levels - 1) < 1:
            raise ValueError("an image of %d x %d has no pixel at pyramid level %d (pair %d)" % (w, h, opt.n_levels - 1, k))
        fx, fy, cx, cy = K[k]
        if not (math.isfinite(fx) and math.isfinite(fy) and fx > 0 and fy > 0 and math.isfinite(cx) and math.isfinite(cy)):
            raise ValueError("intrinsic: fx and fy must be finite and > 0, cx and cy finite (pair %d)" % k)
        T = np.array(np.eye(4) if inits[k] is None else inits[k], dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise ValueError("init must be a finite 4 x 4 matrix (pair %d)" % k)
        r = recs[k]
        r.width, r.height, r.depth_format = w, h, (0 if sd.dtype == np.uint16 else 1)
        for name, (a, px) in zip(("source_depth", "target_depth"), imgs):
            setattr(r, name + "_row_bytes", a.strides[0] if a.size else a.shape[1] * px)
        r.fx, r.fy, r.cx, r.cy = fx, fy, cx, cy
        r.init[:] = list(T.ravel())
        r.depth_scale = float(option.depth_scale)
        for p, (a, _) in zip(ptrs, imgs):
            p[k] = a.ctypes.data_as(_vp)
            keep.append(a)
    return b, recs, opt, ptrs, keep


def compute_depth_odometry_batch(source_depths, target_depths, intrinsic, init=None, option=None, return_trace=False,
                                 device=-1):
    """Per pair a DepthOdometryResult, all pairs in one launch sequence (include/teaser_hip.h, "Depth odometry"): the
    point-to-plane odometry of Open3D's tensor API on depth images alone.  source_depths, target_depths: lists of
    height x width uint16 or float32 arrays; intrinsic, init: one for all pairs or a list with one per pair."""
    from . import lib
    b, recs, opt, ptrs, keep = _depth_pairs(source_depths, target_depths, intrinsic, init,
                                            DepthOdometryOption() if option is None else option)
    if b == 0:
        return []
    n_iter = sum(opt.iterations[k] for k in range(opt.n_levels))
    res = (DepthOdometryResultC * b)()
    traces = [(DepthOdometryTraceC * max(n_iter, 1))() for _ in range(b)] if return_trace else None
    tp = (_vp * b)(*[C.cast(t, _vp) for t in traces]) if return_trace else None
    _handle(device).call(lib().teaser_hip_icp_depth_odometry_pairs, b, recs, C.byref(opt), *ptrs, res, tp)
    out = []
    for k in range(b):
        r = res[k]
        tr = DepthOdometryTrace((DepthOdometryTraceC * n_iter).from_buffer(traces[k]) if n_iter else b"") if return_trace else None
        out.append(DepthOdometryResult(bool(r.success), np.array(r.transformation[:]).reshape(4, 4),
                                       np.array(r.information[:]).reshape(6, 6), float(r.fitness), float(r.inlier_rmse),
                                       int(r.count), int(r.iterations), int(r.converged_levels), tr))
    return out


def compute_depth_odometry(source_depth, target_depth, intrinsic, init=None, option=None, device=-1):
    """One pair: the DepthOdometryResult (success, transformation, information, fitness, inlier_rmse)."""
    return compute_depth_odometry_batch([source_depth], [target_depth], intrinsic, init, option, device=device)[0]


def depth_odometry_pyramid_batch(source_depths, target_depths, intrinsic, option=None, device=-1):
    """The preprocessing stage alone, by the kernels the odometry runs: per pair a list of levels, each a dict of float32
    images D_s, D_t (height x width) and source_vertex, target_vertex, target_normal (height x width x 3)."""
    from . import lib
    b, recs, opt, ptrs, keep = _depth_pairs(source_depths, target_depths, intrinsic, None,
                                            DepthOdometryOption() if option is None else option)
    if b == 0:
        return []
    L = opt.n_levels
    dims = [[(recs[k].height >> l, recs[k].width >> l) for l in range(L)] for k in range(b)]
    flat = [np.empty(len(DEPTH_PLANES) * sum(h * w for h, w in dims[k]), dtype=np.float32) for k in range(b)]
    out_ptrs = (_vp * b)(*[a.ctypes.data_as(_vp) for a in flat])
    _handle(device).call(lib().teaser_hip_icp_depth_odometry_pyramid_pairs, b, recs, C.byref(opt), *ptrs, out_ptrs)
    out = []
    for k in range(b):
        at, levels = 0, []
        for h, w in dims[k]:
            pl = [flat[k][at + i * h * w: at + (i + 1) * h * w].reshape(h, w) for i in range(len(DEPTH_PLANES))]
            levels.append(dict(D_s=pl[0], D_t=pl[1], source_vertex=np.stack(pl[2:5], axis=2),
                               target_vertex=np.stack(pl[5:8], axis=2), target_normal=np.stack(pl[8:11], axis=2)))
            at += len(DEPTH_PLANES) * h * w
        out.append(levels)
    return out


class TrackingResult:
    """What track_frame_to_model returns: camera_to_world (the tracked pose of the frame), result (the
    DepthOdometryResult of the frame against the model view) and model_depth (the ray-cast depth the frame was tracked
    against, float32 metres, 0 where the model has no surface)."""

    def __init__(self, camera_to_world, result, model_depth):
        self.camera_to_world, self.result, self.model_depth = camera_to_world, result, model_depth

    @property
    def success(self):
        return self.result.success


def track_frame_to_model(volume, depth, intrinsic, camera_to_world_init, option=None, weight_threshold=1.0, device=-1):
    """Frame-to-model tracking (Open3D's t.pipelines.slam.Model.track_frame_to_model) against a UniformTSDFVolume or a
    ScalableTSDFVolume of any colour type.  The model's depth map is ray cast at the initial pose -- the ray cast's
    ``extrinsic`` is world-to-camera, so it is given the inverse of camera_to_world_init -- with the frame's intrinsic and
    size; depth odometry then runs with the input frame as SOURCE, the model view as TARGET and the identity as init.  Its
    T takes a point of the frame's camera to the camera of the initial pose, so the frame's pose is
    camera_to_world_init @ T.  The ray-cast map comes back to the host and goes up again with the frame: the TSDF and
    the ICP handle share no device memory.  option: a DepthOdometryOption; its depth_min and depth_max also bound the
    ray cast (the ray cast needs depth_min > 0: 0.1 is used when the option's is smaller)."""
    option = DepthOdometryOption() if option is None else option
    if not isinstance(option, DepthOdometryOption):
        raise ValueError("option must be a DepthOdometryOption")
    E = np.array(camera_to_world_init, dtype=np.float64)
    if E.shape != (4, 4) or not np.isfinite(E).all():
        raise ValueError("camera_to_world_init must be a finite 4 x 4 matrix")
    frame = np.asarray(depth)
    if frame.ndim != 2:
        raise ValueError("depth has shape %s" % (frame.shape,))
    if frame.dtype == np.uint16:  # both images of a pair share the format: the model's view is float32 metres
        frame = frame.astype(np.float32) / np.float32(option.depth_scale)
    h, w = frame.shape
    view = volume.ray_cast_batch(intrinsic, [np.linalg.inv(E)], w, h, depth_min=max(float(option.depth_min), 0.1),
                                 depth_max=float(option.depth_max), weight_threshold=weight_threshold, vertex_map=False,
                                 normal_map=False, color=False)[0]
    r = compute_depth_odometry(frame, view.depth, intrinsic, None, option, device=device)
    return TrackingResult(E @ r.transformation, r, view.depth)


__all__ = ["OdometryOption", "RGBDOdometryJacobianFromColorTerm", "RGBDOdometryJacobianFromHybridTerm", "RGBDImage",
           "OdometryResult", "OdometryTrace", "compute_rgbd_odometry", "compute_rgbd_odometry_batch",
           "rgbd_odometry_pyramid_batch", "OdometryConvergenceCriteria", "OdometryLossParams", "DepthOdometryOption",
           "DepthOdometryResult", "DepthOdometryTrace", "TrackingResult", "compute_depth_odometry",
           "compute_depth_odometry_batch", "depth_odometry_pyramid_batch", "track_frame_to_model"]
