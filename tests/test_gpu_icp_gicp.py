"""Batched Generalized ICP and the covariance estimation on the MI355X against the numpy restatement of the contract
(tests/icp_gicp_reference.py): equal correspondence sets, iteration counts and fitness (the fixture's generator asserts
the decision margins that make this a fair demand), transforms within 1e-9, RMSE within 1e-12 relative; estimated
covariances within a bar derived per point from its eigenvalues; a problem inside a batch that mixes the three methods
gives the same bits as alone; point-to-point and point-to-plane keep their bits through the _cov entry points; invalid
arguments are refused with the argument named.

The 1e-9 bar on ||dT||_F: measured on the CPU with the restatement on config 5 (A and g summed in two shuffled orders,
and in chunks of 256 source points, against ascending order): ||dT||_F between 4.4e-17 and 2.3e-16, RMSE 1.5e-16 to
4.4e-16 relative, iteration count (5) and correspondence set unchanged.  Ten times that is seven orders below 1e-9, so
the project's existing bar stands."""
import ctypes as C
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import icp_gicp_reference as RG
import icp_plane_reference as RP
import icp_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")

# max |dC| <= 2 |dn|, |dn| <= |dcov| / (lambda1 - lambda0), |dcov| <= (m + the Jacobi iteration's few tens) ulps of
# lambda2 with m <= 100 summed neighbours: c = 2 * 256 covers both clouds' worst case
COV_C = 512.0


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


GICP = tp.TransformationEstimationForGeneralizedICP


def assert_matches(gpu, ref):
    print("iterations %d / %d  |C| %d / %d  dT %.3g  dfit %.3g  drmse(rel) %.3g" % (
        gpu.iterations, ref["iterations"], len(gpu.correspondence_set), len(ref["correspondence_set"]),
        np.linalg.norm(gpu.transformation - ref["transformation"]), abs(gpu.fitness - ref["fitness"]),
        abs(gpu.inlier_rmse - ref["inlier_rmse"]) / max(ref["inlier_rmse"], 1e-300)))
    assert gpu.iterations == ref["iterations"]
    assert np.array_equal(gpu.correspondence_set, ref["correspondence_set"])
    assert gpu.fitness == ref["fitness"]
    assert np.linalg.norm(gpu.transformation - ref["transformation"]) < 1e-9
    assert abs(gpu.inlier_rmse - ref["inlier_rmse"]) <= 1e-12 * max(ref["inlier_rmse"], 1e-300)


def same_bits(a, b):
    return (a.transformation.tobytes() == b.transformation.tobytes() and a.fitness == b.fitness and
            a.inlier_rmse == b.inlier_rmse and a.iterations == b.iterations and
            np.array_equal(a.correspondence_set, b.correspondence_set))


def curved_pair(seed=21, n=70):
    """The pair of tests/test_gpu_icp_plane.py (a curved surface, noise, 20 % outliers with random normals), with the
    analytic normals of BOTH clouds (the source's rotated back with it)."""
    rng = np.random.default_rng(seed)
    g = (2.0 / n) * np.arange(n) - 1.0
    x, y = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    S = np.stack([x, y, 0.2 * np.sin(2 * x) * np.cos(1.5 * y)], 1)
    zx, zy = 0.4 * np.cos(2 * x) * np.cos(1.5 * y), -0.3 * np.sin(2 * x) * np.sin(1.5 * y)
    N = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    T_true = pose([0.2, -0.4, 1.0], 1.0, [0.006, -0.004, 0.005])
    P = R.apply(np.linalg.inv(T_true), S)
    Np = N @ T_true[:3, :3]  # rows R^T n
    Q = S + rng.normal(0, 0.002, size=S.shape)
    Nq = N.copy()
    out = rng.permutation(len(Q))[: len(Q) // 5]
    Q[out] = rng.uniform([-1, -1, -0.3], [1, 1, 0.3], size=(len(out), 3))
    rn = rng.normal(size=(len(out), 3))
    Nq[out] = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    return P, Q, Np, Nq, T_true


def test_curved_surface_matches_the_restatement():
    P, Q, Np, Nq, T_true = curved_pair()
    Cs, Ct = tp.covariances_from_normals(Np, 1e-3), tp.covariances_from_normals(Nq, 1e-3)
    assert np.array_equal(Cs, RG.covariances_from_normals(Np, 1e-3))
    ref = RG.registration_icp(P, Q, Cs, Ct, 0.03, np.eye(4))
    gpu = tp.registration_icp(P, Q, 0.03, np.eye(4), GICP(), source_covariances=Cs, target_covariances=Ct)
    assert_matches(gpu, ref)
    assert gpu.iterations >= 2 and gpu.fitness > 0.7 and np.linalg.norm(gpu.transformation - T_true) < 0.01
    # the lower triangle is never read
    junk = Cs.copy()
    junk[:, 1, 0] = junk[:, 2, 0] = junk[:, 2, 1] = np.nan
    again = tp.registration_icp(P, Q, 0.03, np.eye(4), GICP(), source_covariances=junk, target_covariances=Ct)
    assert same_bits(again, gpu)


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "icp_gicp_golden.npz"))


def test_config5_refinement_matches_the_fixture():
    P, Q, r, init = R.config5_problem()
    g = golden()
    Cs, Ct = RG.config5_covariances()
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    gpu = tp.registration_icp(P, Q, r, init, GICP(), crit, source_covariances=Cs, target_covariances=Ct)
    ref = dict(transformation=g["transformation"], correspondence_set=g["correspondence_set"],
               fitness=float(g["fitness"]), inlier_rmse=float(g["inlier_rmse"]), iterations=int(g["iterations"]))
    assert_matches(gpu, ref)
    assert gpu.fitness >= float(g["init_fitness"])
    zero = tp.registration_icp(P, Q, r, init, GICP(), tp.ICPConvergenceCriteria(max_iteration=0),
                               source_covariances=Cs, target_covariances=Ct)
    j, _, fit, rmse = R.corr(R.apply(init, P), Q, r)
    assert zero.iterations == 0 and np.array_equal(zero.transformation, init)
    assert np.array_equal(zero.correspondence_set[:, 0], np.nonzero(j >= 0)[0])
    assert np.array_equal(zero.correspondence_set[:, 1], j[j >= 0])
    assert abs(zero.fitness - fit) <= 1e-12 * fit and abs(zero.inlier_rmse - rmse) <= 1e-12 * rmse
    # registration_generalized_icp estimates what it is not given, on the GPU
    auto = tp.registration_generalized_icp(P, Q, r, init, GICP(), crit, search_radius=float(g["radius"]),
                                           max_nn=int(g["max_nn"]))
    half = tp.registration_generalized_icp(P, Q, r, init, GICP(), crit, source_covariances=Cs,
                                           search_radius=float(g["radius"]), max_nn=int(g["max_nn"]))
    assert same_bits(auto, half)
    assert auto.iterations == ref["iterations"] and np.array_equal(auto.correspondence_set, ref["correspondence_set"])
    assert auto.fitness == ref["fitness"]


def check_covariances(gpu, ref, lam, skip=()):
    """max |dC| per point against COV_C 2^-52 lambda2 / (lambda1 - lambda0); the identity must be exact."""
    ident = np.isnan(lam[:, 0])
    assert np.array_equal(gpu[ident], np.tile(np.eye(3), (int(ident.sum()), 1, 1)))
    assert np.array_equal(gpu, np.transpose(gpu, (0, 2, 1)))
    keep = ~ident
    keep[np.asarray(skip, dtype=np.int64)] = False
    bar = COV_C * 2.0 ** -52 * lam[keep, 2] / (lam[keep, 1] - lam[keep, 0])
    err = np.abs(gpu[keep] - ref[keep]).max(axis=(1, 2))
    print("covariances: %d points, %d identity, max err %.3g, max err / bar %.3g, exact %d" % (
        len(gpu), ident.sum(), err.max(), (err / bar).max(), int((err == 0).sum())))
    assert (err <= bar).all()


def test_estimated_covariances_match_the_restatement_on_the_fixture_clouds():
    P, Q, r, _ = R.config5_problem()
    g = golden()
    both = tp.estimate_covariances_batch([P, Q], float(g["radius"]), int(g["max_nn"]), float(g["epsilon"]))
    for X, got, name in ((P, both[0], "source"), (Q, both[1], "target")):
        ref, N, _, _, lam = RG.estimate_covariances(X, float(g["radius"]), int(g["max_nn"]), float(g["epsilon"]),
                                                   details=True)
        assert np.array_equal(N, g[name + "_normals"])  # the fixture is what the restatement gives
        check_covariances(got, ref, lam, g[name + "_excluded"])
        alone = tp.estimate_covariances(X, float(g["radius"]), int(g["max_nn"]), float(g["epsilon"]))
        assert alone.tobytes() == got.tobytes()
    assert (np.isnan(RG.estimate_covariances(P, 0.1, 20, 1e-3, details=True)[4][:, 0])).sum() >= 1  # identity rows exist


def slab_lattice():
    """A 12 x 12 x 2 lattice with spacing 1/4 (every coordinate and every d2 exact, so neighbours tie exactly) plus
    three far points with fewer than 3 neighbours."""
    g = 0.25 * np.arange(12.0)
    X = np.stack([a.ravel() for a in np.meshgrid(g, g, 0.25 * np.arange(2.0), indexing="ij")], 1)
    return np.concatenate([X, [[50.0, 0, 0], [50.125, 0, 0], [-70.0, 3, 3]]])


def test_lattice_ties_go_to_the_smaller_index_and_sparse_points_get_the_identity():
    X = slab_lattice()
    radius = 0.25 * np.sqrt(2.5)  # self, 5 neighbours at h^2 and 8 at 2 h^2 for an interior point: 14
    for max_nn in (8, 100):  # binding (two of the eight tied neighbours kept: the smaller indices), not binding
        ref, _, nn_gap, _, lam = RG.estimate_covariances(X, radius, max_nn, 1e-3, details=True)
        assert ((nn_gap == 0).sum() > 100) == (max_nn == 8)
        with np.errstate(invalid="ignore"):
            well = (lam[:, 1] - lam[:, 0]) / lam[:, 2] >= 1e-6
        assert well.sum() >= len(X) // 2 and np.isnan(lam[-3:, 0]).all()
        got = tp.estimate_covariances(X, radius, max_nn, 1e-3)
        check_covariances(got, ref, lam, np.nonzero(~well & ~np.isnan(lam[:, 0]))[0])
        perm = np.random.default_rng(max_nn).permutation(len(X))  # another index order: other ties win
        ref_p, _, _, _, lam_p = RG.estimate_covariances(X[perm], radius, max_nn, 1e-3, details=True)
        moved = np.abs(ref_p - ref[perm]).max(axis=(1, 2)) > 1e-3
        assert (moved.sum() > 50) == (max_nn == 8)  # with max_nn binding the index order decides the neighbourhood
        check_covariances(tp.estimate_covariances(X[perm], radius, max_nn, 1e-3), ref_p, lam_p)
    eps = tp.estimate_covariances(X, radius, 8, 0.25)
    k = int(np.nonzero(~np.isnan(lam[:, 0]))[0][0])
    assert abs(np.linalg.eigvalsh(eps[k])[0] - 0.25) < 1e-12 and abs(np.trace(eps[k]) - 2.25) < 1e-12


def mixed_batch():
    """70 problems: 64 config-5 pairs from perturbed seeds cycling through point-to-point, point-to-plane (L2, Tukey)
    and Generalized ICP at three radii, then Generalized ICP with an empty source, an empty target, no correspondence
    at all, all covariances zero (M singular everywhere), identity covariances, and a point-to-plane problem."""
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    Cs, Ct = RG.config5_covariances()
    rng = np.random.default_rng(2026)
    plane = tp.TransformationEstimationPointToPlane
    ests = [GICP(), None, plane(), GICP(), plane(tp.TukeyLoss(0.025)), tp.TransformationEstimationPointToPoint(),
            GICP(), plane(tp.HuberLoss(0.01))]
    rows = []

    def add(s, d, rr, T, e, cs=None, ct=None):
        is_plane, is_gicp = isinstance(e, plane), isinstance(e, GICP)
        rows.append((s, d, rr, T, e, N[:len(d)] if is_plane else None, cs if is_gicp else None,
                     ct if is_gicp else None))

    for k in range(64):
        T = pose(rng.normal(size=3), rng.uniform(0, 3), rng.normal(0, 0.02, 3)) @ init
        add(P, Q, r * (1.0, 1.5, 2.0)[k % 3], T, ests[k % 8], Cs, Ct)
    add(P[:0], Q, r, init, GICP(), Cs[:0], Ct)                                  # 64: n_s = 0
    add(P, Q[:0], r, init, GICP(), Cs, Ct[:0])                                  # 65: n_t = 0
    far = init.copy()
    far[:3, 3] += 100.0
    add(P, Q, r, far, GICP(), Cs, Ct)                                           # 66: no correspondence at all
    add(P, Q, r, init, GICP(), np.zeros_like(Cs), np.zeros_like(Ct))            # 67: M singular everywhere
    eye_s, eye_t = np.tile(np.eye(3), (len(P), 1, 1)), np.tile(np.eye(3), (len(Q), 1, 1))
    add(P, Q, r, init, GICP(), eye_s, eye_t)                                    # 68: isotropic
    add(P, Q, r, init, plane(tp.TukeyLoss(0.025)))                              # 69
    return [list(c) for c in zip(*rows)]


def test_mixed_batch_is_bit_identical_to_single_runs_and_repeatable():
    srcs, dsts, rs, inits, es, nrms, css, cts = mixed_batch()
    assert len(srcs) >= 64
    crit = tp.ICPConvergenceCriteria(max_iteration=50)
    kw = dict(estimation_methods=es, target_normals=nrms, source_covariances=css, target_covariances=cts)
    batch = tp.registration_icp_batch(srcs, dsts, rs, inits, crit, **kw)
    again = tp.registration_icp_batch(srcs, dsts, rs, inits, crit, **kw)
    assert all(same_bits(x, y) for x, y in zip(batch, again))
    for k in range(len(srcs)):
        alone = tp.registration_icp(srcs[k], dsts[k], rs[k], inits[k], es[k], crit, target_normals=nrms[k],
                                    source_covariances=css[k], target_covariances=cts[k])
        assert same_bits(batch[k], alone), k
    assert batch[64].fitness == 0 and batch[65].fitness == 0 and batch[66].fitness == 0
    assert len(batch[66].correspondence_set) == 0 and batch[66].iterations == 1
    # all-zero covariances: nothing enters A, the first pivot fails, U = identity, the loop stops by its own rule
    assert batch[67].iterations == 1 and np.array_equal(batch[67].transformation, inits[67]) and batch[67].fitness > 0
    assert batch[68].iterations >= 2 and batch[68].fitness > 0.5
    assert batch[0].iterations >= 2 and not same_bits(batch[0], batch[1])


def solve(entry, P, Q, r, init, max_iteration, est=None, normals=None, cs=None, ct=None):
    """teaser_hip_icp_solve / _solve_ex / _solve_cov directly: (rc, message, result record, pairs)."""
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    dp = C.POINTER(C.c_double)
    P, Q = np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(Q, dtype=np.float64)
    init = np.ascontiguousarray(init, dtype=np.float64)
    corr = np.zeros((max(len(P), 1), 2), dtype=np.int32)
    p = tp.icp.IcpParamsC(r, max_iteration, 1e-6, 1e-6)
    out = tp.icp.IcpResultC()
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (normals, cs, ct)]
    ptr = [None if a is None else a.ctypes.data_as(dp) for a in keep]
    e = None if est is None else tp.icp.IcpEstimationC(*est)
    args = [h, P.ctypes.data_as(dp), len(P), Q.ctypes.data_as(dp), len(Q), init.ctypes.data_as(dp), C.byref(p),
            C.byref(out), corr.ctypes.data_as(C.POINTER(C.c_int32))]
    if entry != "solve":
        args += [ptr[0], None if e is None else C.byref(e)]
    if entry == "solve_cov":
        args += [ptr[1], ptr[2]]
    with lock:
        rc = getattr(L, "teaser_hip_icp_" + entry)(*args)
        msg = L.teaser_hip_icp_last_error(h).decode()
    return rc, msg, out, corr[:out.n_correspondences].copy()


def test_point_and_plane_keep_their_bits_through_the_cov_entries():
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    Cs, Ct = RG.config5_covariances()
    rc0, _, o0, c0 = solve("solve", P, Q, r, init, 100)
    assert rc0 == 0 and o0.iterations == 19  # tests/golden/icp_golden.npz
    rc1, _, o1, c1 = solve("solve_ex", P, Q, r, init, 100, (1, 4, 0.025), N)
    assert rc1 == 0 and o1.iterations >= 1
    for est, nv, cs, ct in ((None, None, None, None), ((0, 0, 1.0), None, None, None), ((0, 0, 1.0), N, Cs, Ct)):
        rc, msg, o, c = solve("solve_cov", P, Q, r, init, 100, est, nv, cs, ct)
        assert rc == 0, msg
        assert bytes(o) == bytes(o0) and np.array_equal(c, c0), est
    for cs, ct in ((None, None), (Cs, Ct)):
        rc, msg, o, c = solve("solve_cov", P, Q, r, init, 100, (1, 4, 0.025), N, cs, ct)
        assert rc == 0, msg
        assert bytes(o) == bytes(o1) and np.array_equal(c, c1)
    # inside a batch whose first problem is Generalized ICP (the third instantiation)
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    plane = tp.TransformationEstimationPointToPlane(tp.TukeyLoss(0.025))
    mixed = tp.registration_icp_batch([P, P, P], [Q, Q, Q], r, init, crit, estimation_methods=[GICP(), None, plane],
                                      target_normals=[None, None, N], source_covariances=[Cs, None, None],
                                      target_covariances=[Ct, None, None])
    for got, o, c in ((mixed[1], o0, c0), (mixed[2], o1, c1)):
        assert got.transformation.tobytes() == bytes(o)[:128] and got.fitness == o.fitness
        assert got.inlier_rmse == o.inlier_rmse and got.iterations == o.iterations
        assert np.array_equal(got.correspondence_set, c)
    # the older entries still refuse method 2
    rc, msg, _, _ = solve("solve_ex", P, Q, r, init, 100, (2, 0, 1.0), N)
    assert rc == 1 and "method" in msg


def test_far_from_the_origin():
    """The config-5 pair and its seed moved by s = (1e5, -2e5, 3e4) m (the shift of the other two ICP suites);
    covariances do not move with a translation.  Bars as there: the rotation, and the translation expressed in the
    un-shifted frame, at ten times the larger of two differences MEASURED ON THE CPU with the restatement before any
    GPU run:
      shifted vs un-shifted run                      ||dR||_F 3.6e-12, dt 2.3e-11 m, rmse 6.7e-12 relative
      shifted run, sums in chunks of 256 source
      points vs ascending order                      ||dR||_F 4.8e-12, dt 1.5e-11 m, rmse 7.0e-12 relative
    In both, fitness, correspondence set and iteration count (5) are equal; decision margins of the shifted run:
    best / second-best 2.7e-5, radius 1.5e-6, stop rule 8.0e-7.  Bars: ||dR||_F 4.8e-11, dt 2.3e-10 m, rmse 7.1e-11."""
    P, Q, r, init = R.config5_problem()
    Cs, Ct = RG.config5_covariances()
    s = np.array([1e5, -2e5, 3e4])
    shift, unshift = np.eye(4), np.eye(4)
    shift[:3, 3], unshift[:3, 3] = s, -s
    crit = tp.ICPConvergenceCriteria(max_iteration=100)
    init_far = shift @ init @ unshift
    kw = dict(source_covariances=Cs, target_covariances=Ct)
    ref = RG.registration_icp(P + s, Q + s, Cs, Ct, r, init_far, max_iteration=100)
    gpu = tp.registration_icp(P + s, Q + s, r, init_far, GICP(), crit, **kw)
    near = tp.registration_icp(P, Q, r, init, GICP(), crit, **kw)
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
    assert abs(gpu.inlier_rmse - ref["inlier_rmse"]) <= 7.1e-11 * ref["inlier_rmse"]
    assert np.linalg.norm(gpu.transformation[:3, :3] - ref["transformation"][:3, :3]) < 4.8e-11
    assert np.abs(back[:3, 3] - ref_back[:3, 3]).max() < 2.3e-10
    assert np.linalg.norm(back[:3, :3] - near.transformation[:3, :3]) < 4.8e-11
    assert np.abs(back[:3, 3] - near.transformation[:3, 3]).max() < 2.3e-10


def test_invalid_arguments_are_refused():
    rng = np.random.default_rng(0)
    P = rng.uniform(size=(10, 3))
    Cv = np.tile(np.eye(3), (10, 1, 1))
    eye = np.eye(4)

    def usable():
        rc, msg, o, _ = solve("solve_cov", P, P, 0.1, eye, 30, (2, 0, 1.0), None, Cv, Cv)
        assert rc == 0 and o.fitness == 1.0, msg

    usable()
    nan_c, inf_c, low = Cv.copy(), Cv.copy(), Cv.copy()
    nan_c[3, 0, 1], inf_c[9, 2, 2], low[4, 2, 0] = np.nan, np.inf, np.nan
    cases = [(((3, 0, 1.0), Cv, Cv), "method"), (((-1, 0, 1.0), Cv, Cv), "method"), (((2, 1, 0.1), Cv, Cv), "kernel"),
             (((2, 4, 0.1), Cv, Cv), "kernel"), (((2, 5, 1.0), Cv, Cv), "kernel"),
             (((2, 0, 1.0), None, Cv), "src_cov"), (((2, 0, 1.0), Cv, None), "dst_cov"),
             (((2, 0, 1.0), nan_c, Cv), "src_cov"), (((2, 0, 1.0), Cv, inf_c), "dst_cov")]
    for (est, cs, ct), name in cases:
        rc, msg, _, _ = solve("solve_cov", P, P, 0.1, eye, 30, est, None, cs, ct)
        assert rc == 1 and name in msg and "problem 0" in msg, (est, rc, msg)
        usable()
    rc, msg, _, _ = solve("solve_cov", P, P, 0.1, eye, 30, (2, 0, 1.0), None, low, Cv)  # lower triangle: not read
    assert rc == 0, msg
    rc, msg, o, _ = solve("solve_cov", P, P[:0], 0.1, eye, 30, (2, 0, 1.0), None, Cv, None)  # no target: no dst_cov
    assert rc == 0 and o.fitness == 0
    # a batch whose covariance array is given but holds NULL for the Generalized-ICP problem
    L = tp.lib()
    h, lock = tp.icp._handle(-1)
    dp = C.POINTER(C.c_double)
    pp = (dp * 2)(P.ctypes.data_as(dp), P.ctypes.data_as(dp))
    cc = (dp * 2)(Cv.ctypes.data_as(dp), None)
    n2 = np.array([10, 10], dtype=np.int32)
    par = (tp.icp.IcpParamsC * 2)(tp.icp.IcpParamsC(0.1, 30, 1e-6, 1e-6), tp.icp.IcpParamsC(0.1, 30, 1e-6, 1e-6))
    est = (tp.icp.IcpEstimationC * 2)(tp.icp.IcpEstimationC(0, 0, 1.0), tp.icp.IcpEstimationC(2, 0, 1.0))
    out = (tp.icp.IcpResultC * 2)()
    ip = n2.ctypes.data_as(C.POINTER(C.c_int32))
    with lock:
        rc = L.teaser_hip_icp_batch_cov(h, 2, pp, ip, pp, ip, None, par, out, None, None, est, cc, cc)
        msg = L.teaser_hip_icp_last_error(h).decode()
    assert rc == 1 and "src_cov" in msg and "problem 1" in msg
    usable()
    # covariance estimation
    bad = P.copy()
    bad[2, 1] = np.nan
    for kw, name in ((dict(radius=0.0), "radius"), (dict(radius=float("nan")), "radius"),
                     (dict(radius=float("inf")), "radius"), (dict(epsilon=0.0), "epsilon"),
                     (dict(epsilon=float("nan")), "epsilon"), (dict(max_nn=2), "max_nn"), (dict(max_nn=101), "max_nn"),
                     (dict(points=bad), "points"), (dict(points=None), "points"), (dict(out=None), "out")):
        a = dict(points=P, radius=0.3, max_nn=20, epsilon=1e-3, out=np.zeros((10, 9)))
        a.update(kw)
        pts = (dp * 1)(None if a["points"] is None else a["points"].ctypes.data_as(dp))
        op = (dp * 1)(None if a["out"] is None else a["out"].ctypes.data_as(dp))
        n1 = np.array([10], dtype=np.int32)
        with lock:
            rc = L.teaser_hip_icp_covariances_batch(h, 1, pts, n1.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    (C.c_double * 1)(a["radius"]), (C.c_int32 * 1)(a["max_nn"]),
                                                    (C.c_double * 1)(a["epsilon"]), op)
            msg = L.teaser_hip_icp_last_error(h).decode()
        assert rc == 1 and name in msg, (kw, rc, msg)
        usable()
    assert tp.estimate_covariances(P, 0.5).shape == (10, 3, 3) and tp.estimate_covariances(P[:0], 0.5).shape == (0, 3, 3)
    with lock:  # epsilon NULL: 1e-3
        got = np.zeros((10, 9))
        rc = L.teaser_hip_icp_covariances_batch(h, 1, (dp * 1)(P.ctypes.data_as(dp)),
                                                np.array([10], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                                                (C.c_double * 1)(0.5), (C.c_int32 * 1)(20), None,
                                                (dp * 1)(got.ctypes.data_as(dp)))
    assert rc == 0 and np.array_equal(got.reshape(10, 3, 3), tp.estimate_covariances(P, 0.5))
    with pytest.raises(tp.TeaserHipError, match="BAD_ARG"):
        tp.registration_icp(P, P, 0.1, eye, GICP(), source_covariances=nan_c, target_covariances=Cv)


def test_cxx_facade_reproduces_python():
    from icp_gicp_cxx import build_icp_gicp_example
    exe = build_icp_gicp_example()
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 0
    P, Q, r, init = R.config5_problem()
    g = golden()
    Cs, Ct = tp.estimate_covariances_batch([P, Q], float(g["radius"]), int(g["max_nn"]), float(g["epsilon"]))
    py = tp.registration_icp(P, Q, r, init, GICP(), tp.ICPConvergenceCriteria(max_iteration=100),
                             source_covariances=Cs, target_covariances=Ct)
    with tempfile.TemporaryDirectory() as d:
        P.tofile(os.path.join(d, "src.bin"))
        Q.tofile(os.path.join(d, "dst.bin"))
        init.tofile(os.path.join(d, "init.bin"))
        out = subprocess.run([exe, d, repr(r), "100", repr(float(g["radius"])), str(int(g["max_nn"]))],
                             capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    vals = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}
    assert np.array_equal(np.array([float(v) for v in vals["T"]]).reshape(4, 4), py.transformation)
    assert float(vals["fitness"][0]) == py.fitness and float(vals["rmse"][0]) == py.inlier_rmse
    assert int(vals["iterations"][0]) == py.iterations
    assert int(vals["correspondences"][0]) == len(py.correspondence_set)


def test_example_script_refines_with_generalized_icp():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "teaser_python_fpfh.py"), "--icp-gicp",
                          "--gicp-radius", "0.1", "--gicp-max-nn", "20"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("ICP ")]
    before = float(next(ln for ln in lines if "before" in ln).split("fitness")[1].split()[0])
    after = float(next(ln for ln in lines if "after" in ln).split("fitness")[1].split()[0])
    assert after >= before
