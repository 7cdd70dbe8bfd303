"""Batched point-to-plane ICP with robust kernels on the MI355X against the numpy restatement of the contract
(tests/icp_plane_reference.py): equal correspondence sets and iteration counts (the fixture's generator asserts the
decision margins that make this a fair demand), transforms within 1e-9, fitness / RMSE within 1e-12 relative; a problem
inside a batch that mixes methods gives the same bits as alone; point-to-point keeps its bits through the _ex entry
points; invalid arguments are refused with the argument named.

The 1e-9 bar on ||dT||_F: the 6 x 6 solve amplifies summation-order rounding by cond(A).  Measured on the CPU with the
restatement on config 5 (A and g summed in a shuffled order, and in 256-row chunks, against ascending order): ||dT||_F
between 1.1e-16 and 5.2e-16 for L2 and Tukey, iteration counts and correspondence sets unchanged -- seven orders below
the bar, so the project's existing bar stands."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import icp_plane_reference as RP
import icp_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

KERNELS = {"l2": lambda k: tp.L2Loss(), "huber": tp.HuberLoss, "cauchy": tp.CauchyLoss, "gm": tp.GMLoss,
           "tukey": tp.TukeyLoss}


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = rot(axis, deg)
    T[:3, 3] = t
    return T


def plane(kernel="l2", k=1.0):
    return tp.TransformationEstimationPointToPlane(KERNELS[kernel](k))


def assert_matches(gpu, ref):
    print("iterations %d / %d  |C| %d / %d  dT %.3g  dfit %.3g  drmse(rel) %.3g" % (
        gpu.iterations, ref["iterations"], len(gpu.correspondence_set), len(ref["correspondence_set"]),
        np.linalg.norm(gpu.transformation - ref["transformation"]), abs(gpu.fitness - ref["fitness"]),
        abs(gpu.inlier_rmse - ref["inlier_rmse"]) / max(ref["inlier_rmse"], 1e-300)))
    assert gpu.iterations == ref["iterations"]
    assert np.array_equal(gpu.correspondence_set, ref["correspondence_set"])
    assert np.linalg.norm(gpu.transformation - ref["transformation"]) < 1e-9
    assert abs(gpu.fitness - ref["fitness"]) <= 1e-12 * max(ref["fitness"], 1e-300)
    assert abs(gpu.inlier_rmse - ref["inlier_rmse"]) <= 1e-12 * max(ref["inlier_rmse"], 1e-300)


def same_bits(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.fitness == b.fitness and
            a.inlier_rmse == b.inlier_rmse and a.iterations == b.iterations and
            np.array_equal(a.correspondence_set, b.correspondence_set))


def curved_pair(seed=21, n=70):
    """Source: the surface z = 0.2 sin(2 x) cos(1.5 y) sampled on a grid, moved back by a small pose.  Target: the
    surface points with noise and their analytic normals; 20 % of the targets replaced by points with no counterpart
    (uniform in the box, random unit normals)."""
    rng = np.random.default_rng(seed)
    g = (2.0 / n) * np.arange(n) - 1.0
    x, y = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    S = np.stack([x, y, 0.2 * np.sin(2 * x) * np.cos(1.5 * y)], 1)
    zx, zy = 0.4 * np.cos(2 * x) * np.cos(1.5 * y), -0.3 * np.sin(2 * x) * np.sin(1.5 * y)
    N = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    T_true = pose([0.2, -0.4, 1.0], 1.0, [0.006, -0.004, 0.005])
    P = R.apply(np.linalg.inv(T_true), S)
    Q = S + rng.normal(0, 0.002, size=S.shape)
    out = rng.permutation(len(Q))[: len(Q) // 5]
    Q[out] = rng.uniform([-1, -1, -0.3], [1, 1, 0.3], size=(len(out), 3))
    rn = rng.normal(size=(len(out), 3))
    N[out] = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    return P, Q, N, T_true


@pytest.mark.parametrize("kernel,k", [("l2", 1.0), ("huber", 0.004), ("cauchy", 0.004), ("gm", 0.004),
                                      ("tukey", 0.01)])
def test_curved_surface_matches_the_restatement(kernel, k):
    P, Q, N, T_true = curved_pair()
    ref = RP.registration_icp(P, Q, N, 0.03, np.eye(4), kernel=kernel, k=k)
    gpu = tp.registration_icp(P, Q, 0.03, np.eye(4), plane(kernel, k), target_normals=N)
    assert_matches(gpu, ref)
    assert gpu.iterations >= 2 and gpu.fitness > 0.7 and np.linalg.norm(gpu.transformation - T_true) < 0.01


@pytest.mark.parametrize("kernel", ["l2", "tukey"])
def test_config5_refinement_matches_the_fixture(kernel):
    P, Q, r, init = R.config5_problem()
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_plane_golden.npz"))
    N, k = g["target_normals"], float(g[kernel + "_k"])
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    gpu = tp.registration_icp(P, Q, r, init, plane(kernel, k), crit, target_normals=N)
    ref = dict(transformation=g[kernel + "_transformation"], correspondence_set=g[kernel + "_correspondence_set"],
               fitness=float(g[kernel + "_fitness"]), inlier_rmse=float(g[kernel + "_inlier_rmse"]),
               iterations=int(g[kernel + "_iterations"]))
    assert_matches(gpu, ref)
    assert gpu.fitness >= float(g["init_fitness"])
    zero = tp.registration_icp(P, Q, r, init, plane(kernel, k), tp.ICPConvergenceCriteria(max_iteration=0),
                               target_normals=N)
    j, _, fit, rmse = R.corr(R.apply(init, P), Q, r)
    assert zero.iterations == 0 and np.array_equal(zero.transformation, init)
    assert np.array_equal(zero.correspondence_set[:, 0], np.nonzero(j >= 0)[0])
    assert np.array_equal(zero.correspondence_set[:, 1], j[j >= 0])
    assert abs(zero.fitness - fit) <= 1e-12 * fit and abs(zero.inlier_rmse - rmse) <= 1e-12 * rmse


def mixed_batch():
    """71 problems: 64 config-5 pairs from perturbed seeds cycling through point-to-point and point-to-plane with
    every kernel and three radii, then empty source, empty target, no correspondence at all, all normals zero, all
    normals parallel (singular A), a point-to-point and a point-to-plane dense pair (> 245 k points each)."""
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    rng = np.random.default_rng(2025)
    ests = [None, plane("l2"), plane("huber", 0.01), plane("cauchy", 0.01), plane("gm", 0.01), plane("tukey", 0.025),
            tp.TransformationEstimationPointToPoint(), plane("tukey", 0.05)]
    srcs, dsts, nrms, rs, inits, es = [], [], [], [], [], []

    def add(s, d, n, rr, T, e):
        srcs.append(s), dsts.append(d), nrms.append(n), rs.append(rr), inits.append(T), es.append(e)

    for k in range(64):
        T = pose(rng.normal(size=3), rng.uniform(0, 3), rng.normal(0, 0.02, 3)) @ init
        e = ests[k % 8]
        add(P, Q, N if isinstance(e, tp.TransformationEstimationPointToPlane) else None, r * (1.0, 1.5, 2.0)[k % 3],
            T, e)
    add(P[:0], Q, N, r, init, plane("tukey", 0.025))                       # 64: n_s = 0
    add(P, Q[:0], N[:0], r, init, plane())                                 # 65: n_t = 0
    far = init.copy()
    far[:3, 3] += 100.0
    add(P, Q, N, r, far, plane("huber", 0.01))                             # 66: no correspondence at all
    add(P, Q, np.zeros_like(N), r, init, plane())                          # 67: zero normals
    add(P, Q, np.tile([0.0, 0.0, 1.0], (len(Q), 1)), r, init, plane())     # 68: parallel normals
    rng = np.random.default_rng(5)                                         # dense pair: jittered upsampling
    A = np.repeat(P, 48, axis=0) + rng.normal(0, 0.01, size=(48 * len(P), 3))
    B = np.repeat(Q, 50, axis=0) + rng.normal(0, 0.01, size=(50 * len(Q), 3))
    add(A, B, None, r, init, None)                                         # 69: dense, point-to-point
    add(A, B, np.repeat(N, 50, axis=0), r, init, plane("tukey", 0.025))    # 70: dense, point-to-plane
    return srcs, dsts, nrms, rs, inits, es


def test_mixed_batch_is_bit_identical_to_single_runs_and_repeatable():
    srcs, dsts, nrms, rs, inits, es = mixed_batch()
    assert len(srcs) >= 64 and len(srcs[-1]) > 245000 and len(dsts[-1]) > 245000
    crit = tp.ICPConvergenceCriteria(max_iteration=50)
    batch = tp.registration_icp_batch(srcs, dsts, rs, inits, crit, estimation_methods=es, target_normals=nrms)
    again = tp.registration_icp_batch(srcs, dsts, rs, inits, crit, estimation_methods=es, target_normals=nrms)
    assert all(same_bits(x, y) for x, y in zip(batch, again))
    for k in range(len(srcs)):
        alone = tp.registration_icp(srcs[k], dsts[k], rs[k], inits[k], es[k], crit, target_normals=nrms[k])
        assert same_bits(batch[k], alone), k
    assert batch[64].fitness == 0 and batch[65].fitness == 0 and batch[66].fitness == 0
    assert len(batch[66].correspondence_set) == 0 and batch[66].iterations == 1
    for k in (67, 68):  # U = identity: T stays the seed, the loop stops by its own rule after one iteration
        assert batch[k].iterations == 1 and np.array_equal(batch[k].transformation, inits[k]) and batch[k].fitness > 0
    assert batch[69].fitness > 0.5 and batch[70].fitness > 0.5 and batch[70].iterations >= 1
    assert not same_bits(batch[69], batch[70])


def solve_ex(P, Q, r, init, max_iteration, est, normals, use_ex=True):
    """teaser_hip_icp_solve_ex (or teaser_hip_icp_solve) directly: (rc, message, result record, pairs)."""
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    dp = C.POINTER(C.c_double)
    P, Q = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    init = np.ascontiguousarray(init, dtype=np.float64)
    corr = np.zeros((max(len(P), 1), 2), dtype=np.int32)
    p = tp.icp.IcpParamsC(r, max_iteration, 1e-6, 1e-6)
    out = tp.icp.IcpResultC()
    nv = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
    e = None if est is None else tp.icp.IcpEstimationC(*est)
    args = (h, P.ctypes.data_as(dp), len(P), Q.ctypes.data_as(dp), len(Q), init.ctypes.data_as(dp), C.byref(p),
            C.byref(out), corr.ctypes.data_as(C.POINTER(C.c_int32)))
    with lock:
        if use_ex:
            rc = L.teaser_hip_icp_solve_ex(*args, None if nv is None else nv.ctypes.data_as(dp),
                                           None if e is None else C.byref(e))
        else:
            rc = L.teaser_hip_icp_solve(*args)
        msg = L.teaser_hip_icp_last_error(h).decode()
    return rc, msg, out, corr[:out.n_correspondences].copy()


def test_point_to_point_keeps_its_bits_through_the_ex_entries():
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    rc0, _, o0, c0 = solve_ex(P, Q, r, init, 100, None, None, use_ex=False)
    assert rc0 == 0 and o0.iterations == 19  # tests/golden/icp_golden.npz
    for est, nv in ((None, None), ((0, 0, 1.0), None), ((0, 0, float("nan")), N)):  # kernel_k is ignored for L2
        rc, msg, o, c = solve_ex(P, Q, r, init, 100, est, nv)
        assert rc == 0, msg
        assert bytes(o) == bytes(o0) and np.array_equal(c, c0), est
    # inside a batch whose other problem is point-to-plane (the launches with the wider partials)
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    mixed = tp.registration_icp_batch([P, P], [Q, Q], r, init, crit, estimation_methods=[plane("tukey", 0.025), None],
                                      target_normals=[N, None])[1]
    assert mixed.transformation.tobytes() == bytes(o0)[:128] and mixed.fitness == o0.fitness
    assert mixed.inlier_rmse == o0.inlier_rmse and mixed.iterations == 19
    assert np.array_equal(mixed.correspondence_set, c0)


def test_far_from_the_origin():
    """The config-5 pair, its normals and its seed moved by s = (1e5, -2e5, 3e4) m (the shift of
    test_gpu_icp.py::test_far_from_the_origin), L2 kernel.  A stored coordinate there carries ~3e-11 m of rounding, so
    the bars are those the coordinates allow, built as in that test: the rotation, and the translation expressed in the
    un-shifted frame (un T sh, which removes the 2e5 m lever arm), at ten times the larger of two differences MEASURED
    ON THE CPU with the restatement (the reference's own error; measured before any GPU run):
      shifted vs un-shifted run                      ||dR||_F 4.8e-12, dt 4.4e-11 m, rmse 5.8e-12 relative
      shifted run, A and g summed in 256-row chunks
      vs ascending order (the GPU's shape of sum)    ||dR||_F 5.1e-12, dt 8.7e-11 m, rmse 4.2e-11 relative
    In all of them fitness, correspondence set and iteration count (8) are equal; decision margins of the shifted run:
    best / second-best 2.7e-5, radius 3.8e-6, stop rule 5.8e-7.  Bars: ||dR||_F 5.2e-11, dt 8.8e-10 m, rmse 4.3e-10.
    (Near the origin the same chunked sum moves T by 5e-16: far away a different last bit of U changes how the moved
    points round at 3e-11 m, which is what these figures show.)
    Uncentred normal equations (x x n with |x| ~ 2e5 m) would lose ten digits in A and miss these by orders of
    magnitude; the step about the bounding-box centre does not."""
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    s = np.array([1e5, -2e5, 3e4])
    shift, unshift = np.eye(4), np.eye(4)
    shift[:3, 3], unshift[:3, 3] = s, -s
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    init_far = shift @ init @ unshift
    ref = RP.registration_icp(P + s, Q + s, N, r, init_far, max_iteration=100)
    gpu = tp.registration_icp(P + s, Q + s, r, init_far, plane(), crit, target_normals=N)
    near = tp.registration_icp(P, Q, r, init, plane(), crit, target_normals=N)
    back, ref_back = unshift @ gpu.transformation @ shift, unshift @ ref["transformation"] @ shift
    print("vs restatement: dR_F %.3g dt %.3g drmse(rel) %.3g; vs un-shifted: dR %.3g dt %.3g" % (
        np.linalg.norm(gpu.transformation[:3, :3] - ref["transformation"][:3, :3]),
        np.abs(back[:3, 3] - ref_back[:3, 3]).max(), abs(gpu.inlier_rmse - ref["inlier_rmse"]) / ref["inlier_rmse"],
        np.linalg.norm(back[:3, :3] - near.transformation[:3, :3]),
        np.abs(back[:3, 3] - near.transformation[:3, 3]).max()))
    assert gpu.iterations == ref["iterations"] == near.iterations
    assert np.array_equal(gpu.correspondence_set, ref["correspondence_set"])
    assert np.array_equal(gpu.correspondence_set, near.correspondence_set)
    assert gpu.fitness == ref["fitness"]
    assert abs(gpu.inlier_rmse - ref["inlier_rmse"]) <= 4.3e-10 * ref["inlier_rmse"]
    assert np.linalg.norm(gpu.transformation[:3, :3] - ref["transformation"][:3, :3]) < 5.2e-11
    assert np.abs(back[:3, 3] - ref_back[:3, 3]).max() < 8.8e-10
    assert np.linalg.norm(back[:3, :3] - near.transformation[:3, :3]) < 5.2e-11
    assert np.abs(back[:3, 3] - near.transformation[:3, 3]).max() < 8.8e-10


def test_invalid_arguments_are_refused():
    rng = np.random.default_rng(0)
    P = rng.uniform(size=(10, 3))
    N = rng.normal(size=(10, 3))
    eye = np.eye(4)
    rc, msg, _, _ = solve_ex(P, P, 0.1, eye, 30, (1, 4, 0.1), N)
    assert rc == 0, msg
    nan_n, inf_n = N.copy(), N.copy()
    nan_n[3, 1], inf_n[9, 2] = np.nan, -np.inf
    cases = [(((2, 0, 1.0), N), "method"), (((-1, 0, 1.0), N), "method"), (((1, 5, 1.0), N), "kernel"),
             (((1, -1, 1.0), N), "kernel"), (((0, 1, 0.1), N), "kernel"), (((0, 4, 0.1), None), "kernel"),
             (((1, 1, 0.0), N), "kernel_k"), (((1, 2, -1.0), N), "kernel_k"),
             (((1, 3, float("nan")), N), "kernel_k"), (((1, 4, float("inf")), N), "kernel_k"),
             (((1, 0, 1.0), None), "dst_normals"), (((1, 0, 1.0), nan_n), "dst_normals"),
             (((1, 4, 0.1), inf_n), "dst_normals")]
    for (est, nv), name in cases:
        rc, msg, _, _ = solve_ex(P, P, 0.1, eye, 30, est, nv)
        assert rc == 1 and name in msg, (est, rc, msg)
        rc, msg, _, _ = solve_ex(P, P, 0.1, eye, 30, (1, 4, 0.1), N)  # the handle is usable afterwards
        assert rc == 0, msg
    # a batch whose normals array is given but holds NULL for the point-to-plane problem
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    dp = C.POINTER(C.c_double)
    pp = (dp * 2)(P.ctypes.data_as(dp), P.ctypes.data_as(dp))
    nn = (dp * 2)(N.ctypes.data_as(dp), None)
    n2 = np.array([10, 10], dtype=np.int32)
    par = (tp.icp.IcpParamsC * 2)(tp.icp.IcpParamsC(0.1, 30, 1e-6, 1e-6), tp.icp.IcpParamsC(0.1, 30, 1e-6, 1e-6))
    est = (tp.icp.IcpEstimationC * 2)(tp.icp.IcpEstimationC(0, 0, 1.0), tp.icp.IcpEstimationC(1, 0, 1.0))
    out = (tp.icp.IcpResultC * 2)()
    ip = n2.ctypes.data_as(C.POINTER(C.c_int32))
    with lock:
        rc = L.teaser_hip_icp_batch_ex(h, 2, pp, ip, pp, ip, None, par, out, None, nn, est)
        msg = L.teaser_hip_icp_last_error(h).decode()
    assert rc == 1 and "dst_normals" in msg and "problem 1" in msg
    # no target: normals are not needed; the Python layer reports BAD_ARG as TeaserHipError
    rc, msg, o, _ = solve_ex(P, P[:0], 0.1, eye, 30, (1, 0, 1.0), None)
    assert rc == 0 and o.fitness == 0
    with pytest.raises(tp.TeaserHipError, match="BAD_ARG"):
        tp.registration_icp(P, P, 0.1, eye, plane("tukey", -1.0), target_normals=N)
    assert tp.registration_icp(P, P, 0.1, eye, plane("tukey", 1.0), target_normals=N).fitness == 1.0


def test_cxx_facade_reproduces_python():
    from icp_plane_cxx import build_icp_plane_example
    exe = build_icp_plane_example()
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 0
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    py = tp.registration_icp(P, Q, r, init, plane("tukey", 0.025), tp.ICPConvergenceCriteria(max_iteration=100),
                             target_normals=N)
    with tempfile.TemporaryDirectory() as d:
        P.tofile(os.path.join(d, "src.bin"))
        Q.tofile(os.path.join(d, "dst.bin"))
        N.tofile(os.path.join(d, "normals.bin"))
        init.tofile(os.path.join(d, "init.bin"))
        out = subprocess.run([exe, d, repr(r), "100", "4", "0.025"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    assert np.array_equal(np.array([float(v) for v in vals["T"]]).reshape(4, 4), py.transformation)
    assert float(vals["fitness"][0]) == py.fitness and float(vals["rmse"][0]) == py.inlier_rmse
    assert int(vals["iterations"][0]) == py.iterations
    assert int(vals["correspondences"][0]) == len(py.correspondence_set)


def test_example_script_refines_with_point_to_plane():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "teaser_python_fpfh.py"), "--icp-plane",
                          "--icp-kernel", "tukey", "--icp-kernel-k", "0.025"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("ICP ")]
    before = float(next(ln for ln in lines if "before" in ln).split("fitness")[1].split()[0])
    after = float(next(ln for ln in lines if "after" in ln).split("fitness")[1].split()[0])
    assert after >= before
