"""Pose-graph optimisation on the GPU with the surface of open3d.pipelines.registration: PoseGraph, PoseGraphNode,
PoseGraphEdge, GlobalOptimizationOption, GlobalOptimizationConvergenceCriteria, GlobalOptimizationLevenbergMarquardt
and global_optimization, plus a batched call and the linearisation as a stage call.  The arithmetic is written out in
include/teaser_hip.h, "Pose-graph optimisation"; one workgroup owns a graph and runs both passes in one launch."""
import ctypes as C

import numpy as np

from ._handles import HandleCache

_vp, _ip, _dp, _u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)

MAX_NODES, MAX_EDGES = 128, 16384
RIGHT_TERM, INCREMENT, REL_RESIDUAL, RESIDUAL, MAX_ITERATION, MAX_ITERATION_LM, TRIVIAL = range(7)
STATUS_NAMES = ("RIGHT_TERM", "INCREMENT", "REL_RESIDUAL", "RESIDUAL", "MAX_ITERATION", "MAX_ITERATION_LM", "TRIVIAL")


class PoseGraphOptionC(C.Structure):
    _fields_ = [("max_iteration", C.c_int32), ("max_iteration_lm", C.c_int32),
                ("min_relative_increment", C.c_double), ("min_relative_residual_increment", C.c_double),
                ("min_right_term", C.c_double), ("min_residual", C.c_double), ("upper_scale_factor", C.c_double),
                ("lower_scale_factor", C.c_double), ("max_correspondence_distance", C.c_double),
                ("edge_prune_threshold", C.c_double), ("preference_loop_closure", C.c_double),
                ("reference_node", C.c_int32), ("reserved", C.c_int32)]


class PoseGraphResultC(C.Structure):
    _fields_ = [("F0", C.c_double), ("F", C.c_double), ("mu", C.c_double * 2), ("iterations", C.c_int32 * 2),
                ("trials", C.c_int32 * 2), ("status", C.c_int32), ("n_trace", C.c_int32)]


class PoseGraphTraceC(C.Structure):
    _fields_ = [("lam", C.c_double), ("rho", C.c_double), ("F_new", C.c_double), ("pass_", C.c_int32),
                ("accepted", C.c_int32), ("factorised", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(PoseGraphOptionC) == 88 and C.sizeof(PoseGraphResultC) == 56 and C.sizeof(PoseGraphTraceC) == 40


def declare(L):
    """ctypes signatures of the pose-graph entry points (called by the package's lib())."""
    L.teaser_hip_posegraph_create.argtypes = [C.c_int32, C.POINTER(_vp)]
    L.teaser_hip_posegraph_destroy.argtypes = [_vp]
    L.teaser_hip_posegraph_last_error.argtypes = [_vp]
    L.teaser_hip_posegraph_last_error.restype = C.c_char_p
    L.teaser_hip_posegraph_fill_scratch.argtypes = [_vp, C.c_int32, C.POINTER(C.c_int64)]
    L.teaser_hip_posegraph_option_default.argtypes = [C.POINTER(PoseGraphOptionC)]
    graph = [_ip, _dp, _ip, _ip, _ip, _dp, _dp, _u8p, C.POINTER(PoseGraphOptionC)]
    one = [C.c_int32, _dp, C.c_int32, _ip, _ip, _dp, _dp, _u8p, C.POINTER(PoseGraphOptionC)]
    out = [_dp, _dp, _u8p, C.POINTER(PoseGraphResultC), C.POINTER(PoseGraphTraceC)]
    L.teaser_hip_posegraph_optimize_batch.argtypes = [_vp, C.c_int32] + graph + out + [_ip]
    L.teaser_hip_posegraph_optimize.argtypes = [_vp] + one + out + [C.c_int32]
    L.teaser_hip_posegraph_linearize_batch.argtypes = [_vp, C.c_int32] + graph + [_dp] * 7
    L.teaser_hip_posegraph_linearize.argtypes = [_vp] + one + [_dp] * 7


_cache = HandleCache("teaser_hip_posegraph")


class PoseGraphNode:
    def __init__(self, pose=None):
        self.pose = np.eye(4) if pose is None else np.array(pose, dtype=np.float64)

    def __repr__(self):
        return "PoseGraphNode(pose=%r)" % (self.pose,)


class PoseGraphEdge:
    """transformation aligns the source node's cloud to the target node's; information is the 6 x 6 matrix of
    get_information_matrix_from_point_clouds (rotation block first)."""

    def __init__(self, source_node_id=-1, target_node_id=-1, transformation=None, information=None, uncertain=False,
                 confidence=1.0):
        self.source_node_id, self.target_node_id = int(source_node_id), int(target_node_id)
        self.transformation = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64)
        self.information = np.eye(6) if information is None else np.array(information, dtype=np.float64)
        self.uncertain, self.confidence = bool(uncertain), float(confidence)

    def __repr__(self):
        return "PoseGraphEdge(%d -> %d, uncertain=%s, confidence=%.6g)" % (
            self.source_node_id, self.target_node_id, self.uncertain, self.confidence)


class PoseGraph:
    def __init__(self, nodes=None, edges=None):
        self.nodes = list(nodes) if nodes is not None else []
        self.edges = list(edges) if edges is not None else []

    def __repr__(self):
        return "PoseGraph with %d nodes and %d edges" % (len(self.nodes), len(self.edges))


class GlobalOptimizationOption:
    def __init__(self, max_correspondence_distance=0.03, edge_prune_threshold=0.25, preference_loop_closure=1.0,
                 reference_node=-1):
        self.max_correspondence_distance = float(max_correspondence_distance)
        self.edge_prune_threshold = float(edge_prune_threshold)
        self.preference_loop_closure = float(preference_loop_closure)
        self.reference_node = int(reference_node)


class GlobalOptimizationConvergenceCriteria:
    def __init__(self, max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                 min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0,
                 lower_scale_factor=1.0 / 3.0):
        self.max_iteration, self.max_iteration_lm = int(max_iteration), int(max_iteration_lm)
        self.min_relative_increment = float(min_relative_increment)
        self.min_relative_residual_increment = float(min_relative_residual_increment)
        self.min_right_term, self.min_residual = float(min_right_term), float(min_residual)
        self.upper_scale_factor, self.lower_scale_factor = float(upper_scale_factor), float(lower_scale_factor)


class GlobalOptimizationMethod:
    pass


class GlobalOptimizationLevenbergMarquardt(GlobalOptimizationMethod):
    pass


class GlobalOptimizationGaussNewton(GlobalOptimizationMethod):
    """Named for the surface's sake: global_optimization raises NotImplementedError for it."""


class PoseGraphOptimizationResult:
    """One graph's result: poses (n x 4 x 4), confidence (m), pruned (m bool), F0, F, iterations and trials per pass,
    mu per pass, status (and status_name), trace (rows of pass, lam, rho, F_new, accepted, factorised; as many as
    the call was given room for) and n_trace (the rows the run produced)."""

    def __init__(self, poses, confidence, pruned, rec, trace):
        self.poses, self.confidence, self.pruned = poses, confidence, pruned
        self.F0, self.F = rec.F0, rec.F
        self.iterations, self.trials, self.mu = list(rec.iterations), list(rec.trials), list(rec.mu)
        self.status, self.n_trace, self.trace = int(rec.status), int(rec.n_trace), trace

    @property
    def status_name(self):
        return STATUS_NAMES[self.status]


def _check_method(method):
    if method is not None and not isinstance(method, GlobalOptimizationLevenbergMarquardt):
        raise NotImplementedError("global_optimization implements GlobalOptimizationLevenbergMarquardt only, got %s"
                                  % type(method).__name__)


def _option_c(criteria, option):
    criteria = criteria if criteria is not None else GlobalOptimizationConvergenceCriteria()
    option = option if option is not None else GlobalOptimizationOption()
    if not isinstance(criteria, GlobalOptimizationConvergenceCriteria):
        raise TypeError("criteria must be a GlobalOptimizationConvergenceCriteria")
    if not isinstance(option, GlobalOptimizationOption):
        raise TypeError("option must be a GlobalOptimizationOption")
    o = PoseGraphOptionC()
    for name in ("max_iteration", "max_iteration_lm", "min_relative_increment", "min_relative_residual_increment",
                 "min_right_term", "min_residual", "upper_scale_factor", "lower_scale_factor"):
        setattr(o, name, getattr(criteria, name))
    for name in ("max_correspondence_distance", "edge_prune_threshold", "preference_loop_closure", "reference_node"):
        setattr(o, name, getattr(option, name))
    return o


def _per_graph(value, count, what):
    if isinstance(value, (list, tuple)):
        if len(value) != count:
            raise ValueError("%s: %d values for %d pose graphs" % (what, len(value), count))
        return list(value)
    return [value] * count


def _pack(pose_graphs):
    """The concatenated arrays of the C ABI for a list of PoseGraph objects."""
    n, m, poses, src, tgt, X, L, unc = [], [], [], [], [], [], [], []
    for b, pg in enumerate(pose_graphs):
        if not isinstance(pg, PoseGraph):
            raise TypeError("pose graph %d is a %s, not a PoseGraph" % (b, type(pg).__name__))
        n.append(len(pg.nodes))
        m.append(len(pg.edges))
        for i, node in enumerate(pg.nodes):
            T = np.asarray(node.pose, dtype=np.float64)
            if T.shape != (4, 4):
                raise ValueError("pose graph %d: the pose of node %d must be 4 x 4, got %s" % (b, i, T.shape))
            poses.append(T)
        for k, e in enumerate(pg.edges):
            T, I = np.asarray(e.transformation, dtype=np.float64), np.asarray(e.information, dtype=np.float64)
            if T.shape != (4, 4):
                raise ValueError("pose graph %d: the transformation of edge %d must be 4 x 4, got %s" % (b, k, T.shape))
            if I.shape != (6, 6):
                raise ValueError("pose graph %d: the information of edge %d must be 6 x 6, got %s" % (b, k, I.shape))
            src.append(e.source_node_id)
            tgt.append(e.target_node_id)
            X.append(T)
            L.append(I)
            unc.append(1 if e.uncertain else 0)
    return dict(n=np.array(n, dtype=np.int32), m=np.array(m, dtype=np.int32),
                poses=np.ascontiguousarray(np.array(poses, dtype=np.float64).reshape(-1, 4, 4)),
                src=np.array(src, dtype=np.int32), tgt=np.array(tgt, dtype=np.int32),
                X=np.ascontiguousarray(np.array(X, dtype=np.float64).reshape(-1, 4, 4)),
                L=np.ascontiguousarray(np.array(L, dtype=np.float64).reshape(-1, 6, 6)),
                unc=np.array(unc, dtype=np.uint8))


def _ptr(a, t):
    return a.ctypes.data_as(t) if a.size else C.cast(None, t)


def _graph_args(p, opts):
    return (_ptr(p["n"], _ip), _ptr(p["poses"], _dp), _ptr(p["m"], _ip), _ptr(p["src"], _ip), _ptr(p["tgt"], _ip),
            _ptr(p["X"], _dp), _ptr(p["L"], _dp), _ptr(p["unc"], _u8p), opts)


def global_optimization_batch(pose_graphs, method=None, criteria=None, option=None, device=-1, trace=0):
    """Optimises every PoseGraph of `pose_graphs` in ONE call (a workgroup per graph) and returns one
    PoseGraphOptimizationResult per graph; the graphs themselves are not changed.  criteria / option: one object for
    all graphs or a list with one per graph.  trace: room for that many trial rows per graph."""
    from . import lib
    _check_method(method)
    pose_graphs = list(pose_graphs)
    batch = len(pose_graphs)
    crit, opt = _per_graph(criteria, batch, "criteria"), _per_graph(option, batch, "option")
    opts = (PoseGraphOptionC * max(batch, 1))(*[_option_c(c, o) for c, o in zip(crit, opt)])
    p = _pack(pose_graphs)
    trace = int(trace)
    if trace < 0:
        raise ValueError("trace must be >= 0")
    if batch == 0:
        return []
    nodes, edges = int(p["n"].sum()), int(p["m"].sum())
    poses_out = np.zeros((nodes, 4, 4))
    conf = np.zeros(edges)
    pruned = np.zeros(edges, dtype=np.uint8)
    res = (PoseGraphResultC * batch)()
    rows = (PoseGraphTraceC * max(trace * batch, 1))()
    caps = np.full(batch, trace, dtype=np.int32)
    _cache.get(device).call(lib().teaser_hip_posegraph_optimize_batch, batch, *_graph_args(p, opts),
                            _ptr(poses_out, _dp), _ptr(conf, _dp), _ptr(pruned, _u8p), res,
                            rows if trace else None, _ptr(caps, _ip))
    out, no, mo = [], 0, 0
    for b in range(batch):
        n, m = int(p["n"][b]), int(p["m"][b])
        kept = min(res[b].n_trace, trace)
        tr = [dict(**{"pass": r.pass_}, lam=r.lam, rho=r.rho, F_new=r.F_new, accepted=bool(r.accepted),
                   factorised=bool(r.factorised)) for r in rows[b * trace:b * trace + kept]]
        out.append(PoseGraphOptimizationResult(poses_out[no:no + n].copy(), conf[mo:mo + m].copy(),
                                               pruned[mo:mo + m].astype(bool), res[b], tr))
        no, mo = no + n, mo + m
    return out


def global_optimization(pose_graph, method=None, criteria=None, option=None, device=-1):
    """open3d.pipelines.registration.global_optimization: works IN PLACE -- the node poses are replaced, every edge's
    confidence is set, and the edges pruned after the first pass are removed.  Returns the result record."""
    res = global_optimization_batch([pose_graph], method, criteria, option, device=device)[0]
    for node, T in zip(pose_graph.nodes, res.poses):
        node.pose = np.array(T)
    for edge, c in zip(pose_graph.edges, res.confidence):
        edge.confidence = float(c)
    pose_graph.edges = [e for e, gone in zip(pose_graph.edges, res.pruned) if not gone]
    return res


def linearize_pose_graph(pose_graph, option=None, device=-1):
    """Stage call: the linearisation at the graph's poses with the first pass's mu.  dict(e (m x 6), r, l (m), mu, F,
    H (6n x 6n; the reference node's rows and columns are zero), g (6n))."""
    from . import lib
    p = _pack([pose_graph])
    n, m = int(p["n"][0]), int(p["m"][0])
    opts = (PoseGraphOptionC * 1)(_option_c(None, option))
    e, r, l = np.zeros((m, 6)), np.zeros(m), np.zeros(m)
    mu, F, H, g = np.zeros(1), np.zeros(1), np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    _cache.get(device).call(lib().teaser_hip_posegraph_linearize_batch, 1, *_graph_args(p, opts), _ptr(e, _dp),
                            _ptr(r, _dp), _ptr(l, _dp), _ptr(mu, _dp), _ptr(F, _dp), _ptr(H, _dp), _ptr(g, _dp))
    return dict(e=e, r=r, l=l, mu=float(mu[0]), F=float(F[0]), H=H, g=g)
