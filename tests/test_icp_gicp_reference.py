"""The Generalized-ICP and covariance-estimation contracts (include/teaser_hip.h) as restated in numpy
(tests/icp_gicp_reference.py) against closed forms, the committed fixture against its generator, and the surface of
the GPU implementation that needs no device: names, defaults, ValueErrors, exported symbols, the C++ example."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import icp_gicp_reference as RG
import icp_plane_reference as RP
import icp_reference as R
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def curved_surface(n=40):
    g = (2.0 / n) * np.arange(n) - 1.0
    x, y = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    z = 0.2 * np.sin(2 * x) * np.cos(1.5 * y)
    zx, zy = 0.4 * np.cos(2 * x) * np.cos(1.5 * y), -0.3 * np.sin(2 * x) * np.sin(1.5 * y)
    nv = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    return np.stack([x, y, z], 1), nv / np.linalg.norm(nv, axis=1, keepdims=True)


def small_pose(angle=0.01, t=(0.004, -0.003, 0.002)):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]
    T[:3, 3] = t
    return T


def test_w_equal_n_nT_is_the_point_to_plane_step():
    """With W = n n^T the Generalized-ICP terms are point-to-plane's (J^T n = [x' x n ; n]).  The two restatements
    multiply in a different order (x' x (W column) against (x' x n) n), so they agree to rounding, not bit for bit:
    each entry is a sum of 1600 products of magnitude <= |x'|^2 <= 3, compared at 1e-12 of the largest entry."""
    Q, N = curved_surface()
    P = R.apply(np.linalg.inv(small_pose()), Q)
    c = RP.centre_of(Q)
    W6 = np.stack([N[:, 0] * N[:, 0], N[:, 0] * N[:, 1], N[:, 0] * N[:, 2], N[:, 1] * N[:, 1], N[:, 1] * N[:, 2],
                   N[:, 2] * N[:, 2]], 1)
    tA, tg = RG.terms_from_W(P - c, (P - c) - (Q - c), W6)
    A, g = RG.sum_terms(tA, tg)
    Ap, gp = RP.normal_equations(P, Q, N, c)
    assert np.abs(A - Ap).max() <= 1e-12 * np.abs(Ap).max() and np.abs(g - gp).max() <= 1e-12 * np.abs(gp).max()
    assert np.array_equal(A, A.T)
    U, Up = RP.step_matrix(RP.solve6(A, g), c), RP.plane_step(P, Q, N, c)
    assert np.linalg.norm(U - Up) < 1e-10


def test_thin_target_covariance_converges_to_point_to_plane():
    """Ct = I - (1 - eps) n n^T, Cs = 0: W = I + (1 / eps - 1) n n^T, so eps W = n n^T + eps (I - n n^T) and the step
    (which does not change when W is scaled) tends to the L2 point-to-plane step linearly in eps: to first order the
    difference is eps times the tangential (point-to-point-like) information applied to a step no longer than the
    motion itself, |xi| <= 0.012 here.  Bar: 0.1 eps (|xi| with a factor of ten for the conditioning of A).  Observed
    ||U - U_plane||_F: eps = 1e-3: 5.9e-7, 1e-6: 7.7e-10, 1e-9: 7.9e-13 (printed below)."""
    Q, N = curved_surface()
    P = R.apply(np.linalg.inv(small_pose()), Q)
    c = RP.centre_of(Q)
    Up = RP.plane_step(P, Q, N, c)
    zero = np.zeros((len(P), 6))
    seen = []
    for eps in (1e-3, 1e-6, 1e-9):
        Ct = RG.sym_upper(RG.covariances_from_normals(N, eps))
        U = RG.gicp_step(P, Q, zero, Ct, np.eye(3), c)
        seen.append(np.linalg.norm(U - Up))
        assert seen[-1] < 1e-1 * eps, (eps, seen)
    print("eps 1e-3, 1e-6, 1e-9 -> ||U - U_plane||_F", seen)
    assert seen[2] < seen[1] < seen[0]


def test_pure_translation_with_identity_covariances_is_recovered_in_one_step():
    rng = np.random.default_rng(3)
    Q = rng.uniform(-1, 1, size=(300, 3))
    t = np.array([0.01, -0.02, 0.015])
    P = Q - t
    eye = np.tile(np.eye(3), (300, 1, 1))
    o = RG.registration_icp(P, Q, eye, eye, 0.05, max_iteration=1)
    assert o["fitness"] == 1.0 and np.array_equal(o["correspondence_set"][:, 0], o["correspondence_set"][:, 1])
    assert np.abs(o["transformation"][:3, 3] - t).max() < 1e-14
    assert np.abs(o["transformation"][:3, :3] - np.eye(3)).max() < 1e-13 and o["inlier_rmse"] < 1e-13


def test_singular_m_contributes_nothing_and_the_loop_stops():
    Q, N = curved_surface(20)
    init = small_pose(0.02)
    zero = np.zeros((len(Q), 3, 3))
    o = RG.registration_icp(Q, Q, zero, zero, 0.2, init, max_iteration=30)
    assert o["iterations"] == 1 and np.array_equal(o["transformation"], init) and o["fitness"] > 0
    neg = -np.tile(np.eye(3), (len(Q), 1, 1))  # det < 0
    o = RG.registration_icp(Q, Q, neg, zero, 0.2, init, max_iteration=30)
    assert o["iterations"] == 1 and np.array_equal(o["transformation"], init)
    # half the correspondences singular: the others alone make the step
    C = RG.covariances_from_normals(N, 1e-3)
    half = C.copy()
    half[::2] = 0.0
    W, ok = RG.information(RG.sym_upper(np.zeros_like(C)), RG.sym_upper(half), np.eye(3))
    assert ok.sum() == len(Q) // 2 and not ok[0] and ok[1]
    # only the upper triangle is read
    junk = C.copy()
    junk[:, 1, 0] = junk[:, 2, 0] = junk[:, 2, 1] = np.nan
    assert np.array_equal(RG.sym_upper(junk), RG.sym_upper(C))


def test_small_rigid_motion_of_a_curved_surface_is_recovered():
    Q, N = curved_surface()
    T_true = small_pose()
    P = R.apply(np.linalg.inv(T_true), Q)
    Ct = RG.covariances_from_normals(N, 1e-3)
    Cs = RG.covariances_from_normals(N @ T_true[:3, :3], 1e-3)
    o = RG.registration_icp(P, Q, Cs, Ct, 0.04, max_iteration=50)
    assert o["fitness"] == 1.0 and o["inlier_rmse"] < 1e-6
    assert np.linalg.norm(o["transformation"] - T_true) < 1e-6


def plane_samples(seed, n=400):
    """Points sampled from a known plane through a random pose, with a little noise off the plane."""
    rng = np.random.default_rng(seed)
    Rm = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.normal(0, 1e-3, n)], 1)
    return X @ Rm.T + rng.normal(size=3), Rm[:, 2]


def test_estimated_covariances_match_eigh_on_sampled_planes():
    """The restatement's normal against numpy.linalg.eigh of the same sample covariance.  Bar per point on
    |n x n_eigh| (the sine of the angle, sign-free): c 2^-52 lambda2 / (lambda1 - lambda0) with c = 64: both solvers
    are backward stable, each perturbing the matrix by a few ulps of its norm (Jacobi: <= 16 sweeps x 3 rotations of
    O(1) ulp each, far fewer in practice; LAPACK's tridiagonal QR likewise), and an eigenvector moves by the
    perturbation over its eigen-gap; 64 ulps covers the two together.  The generator asserts the gap of every point."""
    for seed in (1, 2, 3):
        X, normal = plane_samples(seed)
        C, N, nn_gap, _, lam = RG.estimate_covariances(X, 0.35, 20, 1e-3, details=True)
        used = ~np.isnan(lam[:, 0])
        assert used.sum() > 350 and np.isfinite(nn_gap[used]).mean() > 0.5  # max_nn binds for most points
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
        assert (gap[used] > 0.05).all()  # thin neighbourhoods: the smallest eigenvalue is well separated
        tree_r2 = 0.35 * 0.35
        worst = 0.0
        for i in np.nonzero(used)[0]:
            d2 = ((X - X[i]) ** 2).sum(1)
            js = np.lexsort((np.arange(len(X)), d2))
            js = js[d2[js] < tree_r2][:20]
            a = RG.sample_covariance(X, i, js)
            M = np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])
            w, V = np.linalg.eigh(M)
            s = np.linalg.norm(np.cross(N[i], V[:, 0]))
            bar = 64 * 2.0 ** -52 * w[2] / (w[1] - w[0])
            worst = max(worst, s / bar)
            assert s <= bar, (seed, i, s, bar)
            assert np.abs(np.sort(lam[i]) - w).max() <= 64 * 2.0 ** -52 * w[2]
            assert abs(abs(N[i] @ normal) - 1) < 0.05
            ev = np.linalg.eigvalsh(C[i])
            assert abs(ev[0] - 1e-3) < 1e-14 and abs(ev[1] - 1) < 1e-14 and abs(ev[2] - 1) < 1e-14
        print("seed", seed, "worst sine / bar", worst)
    # fewer than 3 neighbours: the identity; the sign of the normal cannot matter
    far = np.array([[0, 0, 0], [0.1, 0, 0], [9.0, 9, 9]])
    assert np.array_equal(RG.estimate_covariances(far, 0.35), np.tile(np.eye(3), (3, 1, 1)))
    v = np.array([0.6, 0.0, 0.8])
    assert np.array_equal(RG.covariance_from_unit_normal(v, 1e-3), RG.covariance_from_unit_normal(-v, 1e-3))


def test_covariances_from_normals_edge_cases():
    N = np.array([[0, 0, 2.0], [0, 0, 0], [np.nan, 1, 0], [1e200, 1e200, 0], [3, 4, 0], [np.inf, 0, 0]])
    for f in (tp.covariances_from_normals, RG.covariances_from_normals):
        C = f(N, 0.5)
        assert C.shape == (6, 3, 3)
        assert np.array_equal(C[0], np.diag([1, 1, 0.5]))
        for k in (1, 2, 3, 5):  # zero, non-finite, n^T n overflows
            assert np.array_equal(C[k], np.eye(3)), k
        assert np.allclose(C[4], np.eye(3) - 0.5 * np.outer([0.6, 0.8, 0], [0.6, 0.8, 0]), atol=1e-15)
    assert np.array_equal(tp.covariances_from_normals(N, 1e-3), RG.covariances_from_normals(N, 1e-3))
    assert tp.covariances_from_normals(np.zeros((0, 3))).shape == (0, 3, 3)
    for eps in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="epsilon"):
            tp.covariances_from_normals(N, eps)
    with pytest.raises(ValueError):
        tp.covariances_from_normals(np.zeros((4, 2)))


def test_golden_file_regenerates():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "mkg", os.path.join(ROOT, "tests", "golden", "make_icp_gicp_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    d = mk.compute()  # asserts the decision margins >= 1e-9 and the excluded share <= 1 % itself
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_gicp_golden.npz"))
    assert sorted(g.files) == sorted(d)
    for k in ("source_normals", "target_normals", "source_excluded", "target_excluded", "correspondence_set"):
        assert g[k].dtype == d[k].dtype and np.array_equal(g[k], d[k]), k
    assert int(g["iterations"]) == int(d["iterations"]) and int(g["max_nn"]) == 20 and float(g["epsilon"]) == 1e-3
    assert np.linalg.norm(g["transformation"] - d["transformation"]) < 1e-12
    for k in ("fitness", "inlier_rmse", "radius", "r"):
        assert abs(float(g[k]) - float(d[k])) <= 1e-12 * abs(float(d[k])), k
    for k in ("margins", "source_margins", "target_margins"):
        assert (g[k] >= 1e-9).all(), k
    assert len(g["source_excluded"]) <= 0.01 * len(g["source_normals"])
    assert len(g["target_excluded"]) <= 0.01 * len(g["target_normals"])
    assert float(g["fitness"]) > float(g["init_fitness"])
    assert int(g["iterations"]) < 8  # fewer than point-to-plane L2 needs on this pair (tests/golden/icp_plane_golden.npz)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "icp_gicp_golden.npz")) < 300 * 1024


def test_public_names_defaults_and_value_errors():
    for name in ("TransformationEstimationForGeneralizedICP", "registration_generalized_icp", "estimate_covariances",
                 "estimate_covariances_batch", "covariances_from_normals"):
        assert name in tp.__all__ and hasattr(tp, name), name
    gicp = tp.TransformationEstimationForGeneralizedICP()
    assert gicp.epsilon == 1e-3 and tp.TransformationEstimationForGeneralizedICP(0.01).epsilon == 0.01
    assert tp.icp._estimation(gicp) == (2, 0, 1.0)
    with pytest.raises(ValueError, match="L2"):
        tp.TransformationEstimationForGeneralizedICP(kernel=tp.TukeyLoss(0.1))
    with pytest.raises(ValueError, match="epsilon"):
        tp.TransformationEstimationForGeneralizedICP(0.0)
    sig = inspect.signature(tp.registration_icp)
    assert list(sig.parameters)[:7] == ["source", "target", "max_correspondence_distance", "init",
                                        "estimation_method", "criteria", "device"]
    for name in ("target_normals", "source_covariances", "target_covariances"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[name].default is None
    bsig = inspect.signature(tp.registration_icp_batch).parameters
    assert bsig["source_covariances"].default is None and bsig["target_covariances"].default is None
    gsig = inspect.signature(tp.registration_generalized_icp).parameters
    assert list(gsig)[:10] == ["source", "target", "max_correspondence_distance", "init", "estimation_method",
                               "criteria", "source_covariances", "target_covariances", "search_radius", "max_nn"]
    assert gsig["max_nn"].default == 20 and gsig["search_radius"].default is None
    esig = inspect.signature(tp.estimate_covariances).parameters
    assert list(esig)[:4] == ["points", "radius", "max_nn", "epsilon"]
    assert esig["max_nn"].default == 20 and esig["epsilon"].default == 1e-3
    # refused before any library call (no device is needed to get these)
    P = np.zeros((5, 3))
    Cv = np.tile(np.eye(3), (5, 1, 1))
    with pytest.raises(ValueError, match="source_covariances"):
        tp.registration_icp(P, P, 0.1, np.eye(4), gicp, target_covariances=Cv)
    with pytest.raises(ValueError, match="target_covariances"):
        tp.registration_icp(P, P, 0.1, np.eye(4), gicp, source_covariances=Cv)
    with pytest.raises(ValueError, match="shape"):
        tp.registration_icp(P, P, 0.1, np.eye(4), gicp, source_covariances=Cv[:4], target_covariances=Cv)
    with pytest.raises(ValueError, match="shape"):
        tp.registration_icp(P, P, 0.1, np.eye(4), gicp, source_covariances=Cv, target_covariances=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="source_covariances"):
        tp.registration_icp_batch([P, P], [P, P], 0.1, estimation_methods=[None, gicp],
                                  source_covariances=[None, None], target_covariances=[None, Cv])
    with pytest.raises(ValueError, match="target_covariances"):
        tp.registration_icp_batch([P, P], [P, P], 0.1, estimation_methods=[None, gicp], source_covariances=[None, Cv])
    with pytest.raises(ValueError, match="search_radius"):
        tp.registration_generalized_icp(P, P, 0.1)
    with pytest.raises(ValueError, match="search_radius"):
        tp.registration_generalized_icp(P, P, 0.1, source_covariances=Cv)
    with pytest.raises(ValueError, match="estimation_method"):
        tp.registration_generalized_icp(P, P, 0.1, np.eye(4), tp.TransformationEstimationPointToPoint(),
                                        source_covariances=Cv, target_covariances=Cv)
    for kw in (dict(max_nn=2), dict(max_nn=101), dict(radius=0.0), dict(radius=np.nan), dict(epsilon=0.0)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            tp.estimate_covariances(P, **dict(dict(radius=0.1), **kw))
    assert tp.icp.MAX_NN_LIMIT == 100


def test_header_declares_and_library_exports_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    L = tp.lib()
    for name in ("teaser_hip_icp_batch_cov", "teaser_hip_icp_solve_cov", "teaser_hip_icp_covariances_batch"):
        assert re.search(r"TEASER_HIP_API int32_t %s\(" % name, text), name
        assert name in tp.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert re.search(r"#define TEASER_HIP_ICP_COV_MAX_NN 100\b", text)
    assert "bit parity with Open3D is not claimed" in text and "L2 ONLY" in text
    assert len(L.teaser_hip_icp_batch_cov.argtypes) == 14 and len(L.teaser_hip_icp_solve_cov.argtypes) == 13
    assert len(L.teaser_hip_icp_covariances_batch.argtypes) == 8
    assert len(L.teaser_hip_icp_batch.argtypes) == 10 and len(L.teaser_hip_icp_batch_ex.argtypes) == 12
    # the pinned layouts and the ABI version are unchanged
    assert C.sizeof(tp.icp.IcpEstimationC) == 16
    assert C.sizeof(tp.icp.IcpParamsC) == 32 and C.sizeof(tp.icp.IcpResultC) == 152
    assert L.teaser_hip_abi_version() == 1
    assert L.teaser_hip_icp_batch_cov(None, 0, None, None, None, None, None, None, None, None, None, None, None,
                                      None) == 1
    assert L.teaser_hip_icp_covariances_batch(None, 0, None, None, None, None, None, None) == 1


def test_gicp_calls_use_the_cov_entry_and_the_others_their_own(monkeypatch):
    calls = []

    class FakeLib:
        def teaser_hip_icp_create(self, device, out):
            out._obj.value = 4096
            return 0

        def teaser_hip_icp_batch(self, *a):
            calls.append(("batch", len(a)))
            return 0

        def teaser_hip_icp_batch_ex(self, *a):
            calls.append(("batch_ex", len(a), [e.method for e in a[-1]]))
            return 0

        def teaser_hip_icp_batch_cov(self, *a):
            calls.append(("batch_cov", len(a), [(e.method, e.kernel, e.kernel_k) for e in a[11]],
                          [bool(p) for p in a[10]], [bool(p) for p in a[12]], [bool(p) for p in a[13]]))
            return 0

        def teaser_hip_icp_covariances_batch(self, h, b, pts, n, radius, max_nn, eps, out):
            calls.append(("covariances", b, [n[k] for k in range(b)], [radius[k] for k in range(b)],
                          [max_nn[k] for k in range(b)], [eps[k] for k in range(b)]))
            return 0

        def teaser_hip_icp_last_error(self, h):
            return b""

        def teaser_hip_icp_destroy(self, h):
            return 0

    monkeypatch.setattr(tp, "lib", lambda: FakeLib())
    monkeypatch.setattr(tp.icp._cache, "handles", {})
    monkeypatch.setattr(tp._handles, "_current_device", lambda: 0)
    P, Q = np.zeros((4, 3)), np.zeros((6, 3))
    Cp, Cq = np.tile(np.eye(3), (4, 1, 1)), np.tile(np.eye(3), (6, 1, 1))
    gicp = tp.TransformationEstimationForGeneralizedICP(0.01)
    tp.registration_icp(P, Q, 0.1)
    tp.registration_icp(P, Q, 0.1, estimation_method=tp.TransformationEstimationPointToPlane(), target_normals=Q)
    tp.registration_icp(P, Q, 0.1, estimation_method=gicp, source_covariances=Cp, target_covariances=Cq.reshape(6, 9))
    tp.registration_icp_batch([P, P, P], [Q, Q, Q], 0.1, target_normals=[None, Q, None],
                              estimation_methods=[gicp, tp.TransformationEstimationPointToPlane(tp.GMLoss(0.5)), None],
                              source_covariances=[Cp, None, None], target_covariances=[Cq, None, None])
    tp.registration_generalized_icp(P, Q, 0.1, np.eye(4), gicp, search_radius=0.3, max_nn=15)
    tp.registration_generalized_icp(P, Q, 0.1, source_covariances=Cp, search_radius=0.3)
    tp.estimate_covariances_batch([P, Q], [0.2, 0.3], 30, 1e-2)
    assert calls == [
        ("batch", 10), ("batch_ex", 12, [1]),
        ("batch_cov", 14, [(2, 0, 1.0)], [False], [True], [True]),
        ("batch_cov", 14, [(2, 0, 1.0), (1, 3, 0.5), (0, 0, 1.0)], [False, True, False], [True, False, False],
         [True, False, False]),
        ("covariances", 2, [4, 6], [0.3, 0.3], [15, 15], [0.01, 0.01]),
        ("batch_cov", 14, [(2, 0, 1.0)], [False], [True], [True]),
        ("covariances", 1, [6], [0.3], [20], [1e-3]),
        ("batch_cov", 14, [(2, 0, 1.0)], [False], [True], [True]),
        ("covariances", 2, [4, 6], [0.2, 0.3], [30, 30], [0.01, 0.01])]


def test_cxx_icp_gicp_example_exits_77_without_device():
    from icp_gicp_cxx import build_icp_gicp_example
    exe = build_icp_gicp_example()
    rc = subprocess.call([exe], stdout=subprocess.DEVNULL, timeout=120)
    assert rc == (0 if tp.device_count() > 0 else 77)
