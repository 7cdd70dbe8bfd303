"""The point-to-plane ICP contract (include/teaser_hip.h, "ICP refinement: point-to-plane") as restated in numpy
(tests/icp_plane_reference.py) against closed forms, the committed fixture against its generator, and the surface of
the GPU implementation that needs no device: names, defaults, ValueErrors, exported symbols, the C++ example."""
import ctypes as C
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import icp_plane_reference as RP
import icp_reference as R
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


def small_pose(angle=0.01, t=(0.004, -0.003, 0.002)):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]
    T[:3, 3] = t
    return T


def curved_surface(n=40):
    """z = 0.2 sin(2 x) cos(1.5 y) on an n x n grid over [-1, 1)^2 with its analytic unit normals."""
    g = (2.0 / n) * np.arange(n) - 1.0
    x, y = [a.ravel() for a in np.meshgrid(g, g, indexing="ij")]
    z = 0.2 * np.sin(2 * x) * np.cos(1.5 * y)
    zx, zy = 0.4 * np.cos(2 * x) * np.cos(1.5 * y), -0.3 * np.sin(2 * x) * np.sin(1.5 * y)
    nv = np.stack([-zx, -zy, np.ones_like(zx)], 1)
    return np.stack([x, y, z], 1), nv / np.linalg.norm(nv, axis=1, keepdims=True)


def test_kernel_weights_at_closed_form_points():
    k = 0.3
    r = np.array([0.0, k, -k, 2 * k])
    assert np.array_equal(RP.weight("l2", k, r), [1, 1, 1, 1])
    assert np.array_equal(RP.weight("huber", k, r), [1, 1, 1, 0.5])
    assert np.allclose(RP.weight("cauchy", k, r), [1, 0.5, 0.5, 0.2], rtol=1e-15)
    assert np.allclose(RP.weight("gm", k, r), [1 / k, k / (k + k * k) ** 2, k / (k + k * k) ** 2,
                                               k / (k + 4 * k * k) ** 2], rtol=1e-15)
    assert np.array_equal(RP.weight("tukey", k, r), [1, 0, 0, 0])
    assert abs(float(RP.weight("tukey", k, k / 2)) - 0.5625) < 1e-15


def test_sliding_along_a_plane_is_a_fixed_point_of_point_to_plane_only():
    g = 0.1 * np.arange(12.0)
    Q = np.stack([a.ravel() for a in np.meshgrid(g, g, indexing="ij")] + [np.zeros(144)], 1)
    N = np.tile([0.0, 0.0, 1.0], (144, 1))
    P = Q + [0.03, 0.02, 0.0]  # displaced along the plane
    j, _, _, _ = R.corr(P, Q, 0.08)
    A, gv = RP.normal_equations(P, Q[j], N[j], RP.centre_of(Q))
    assert (j == np.arange(144)).all() and np.array_equal(gv, np.zeros(6))
    o = RP.registration_icp(P, Q, N, 0.08, max_iteration=1)
    assert o["iterations"] == 1 and np.array_equal(o["transformation"], np.eye(4))
    pp = R.registration_icp(P, Q, 0.08, max_iteration=1)
    assert np.linalg.norm(pp["transformation"][:3, 3] - [-0.03, -0.02, 0.0]) < 1e-12


def test_small_rigid_motion_of_a_curved_surface_is_recovered():
    Q, N = curved_surface()
    T_true = small_pose()
    P = R.apply(np.linalg.inv(T_true), Q)
    for kernel, k in (("l2", 1.0), ("huber", 0.05), ("cauchy", 0.05), ("gm", 0.05), ("tukey", 0.1)):
        o = RP.registration_icp(P, Q, N, 0.04, kernel=kernel, k=k, max_iteration=50)
        assert o["fitness"] == 1.0 and o["inlier_rmse"] < 1e-6, kernel
        assert np.linalg.norm(o["transformation"] - T_true) < 1e-6, kernel
        assert np.array_equal(o["correspondence_set"][:, 0], o["correspondence_set"][:, 1])


def test_step_is_open3ds_rotation_order_and_centred():
    """R = Rz(gamma) Ry(beta) Rx(alpha), and the step about c maps c to c + t'."""
    xi = np.array([0.1, -0.2, 0.3, 0.01, 0.02, -0.03])
    c = np.array([3.0, -2.0, 5.0])
    U = RP.step_matrix(xi, c)

    def rot(axis, a):
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i] = m[j, j] = np.cos(a)
        m[i, j], m[j, i] = -np.sin(a), np.sin(a)
        return m

    assert np.allclose(U[:3, :3], rot(2, xi[2]) @ rot(1, xi[1]) @ rot(0, xi[0]), atol=1e-15)
    assert np.allclose(U[:3, :3] @ c + U[:3, 3], c + xi[3:], atol=1e-14)


def test_solve6_matches_a_dense_solve_and_refuses_bad_pivots():
    rng = np.random.default_rng(4)
    M = rng.normal(size=(20, 6))
    A, g = M.T @ M, rng.normal(size=6)
    assert np.allclose(RP.solve6(A, g), np.linalg.solve(A, -g), rtol=1e-10)
    A0 = A.copy()
    A0[2, :] = A0[:, 2] = 0.0
    assert RP.solve6(A0, g) is None
    assert RP.solve6(-A, g) is None
    An = A.copy()
    An[0, 0] = np.nan
    assert RP.solve6(An, g) is None


def test_parallel_normals_give_the_identity_and_the_loop_stops():
    Q, _ = curved_surface(20)
    N = np.tile([0.0, 0.0, 1.0], (len(Q), 1))
    init = small_pose(0.02)
    o = RP.registration_icp(Q, Q, N, 0.2, init, max_iteration=30)
    assert o["iterations"] == 1 and np.array_equal(o["transformation"], init) and o["fitness"] > 0
    z = RP.registration_icp(Q, Q, np.zeros_like(Q), 0.2, init, max_iteration=30)  # zero normals: A = 0
    assert z["iterations"] == 1 and np.array_equal(z["transformation"], init)


def test_shifting_both_clouds_keeps_correspondences_and_iterations():
    P, Q, r, init = R.config5_problem()
    N = RP.config5_normals()
    s = np.array([1e3, -2e3, 3e2])
    sh, un = np.eye(4), np.eye(4)
    sh[:3, 3], un[:3, 3] = s, -s
    near = RP.registration_icp(P, Q, N, r, init, max_iteration=100)
    far = RP.registration_icp(P + s, Q + s, N, r, sh @ init @ un, max_iteration=100)
    assert far["iterations"] == near["iterations"]
    assert np.array_equal(far["correspondence_set"], near["correspondence_set"])
    back = un @ far["transformation"] @ sh
    assert np.abs(back - near["transformation"]).max() < 1e-8


def test_golden_file_regenerates():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "mkp", os.path.join(ROOT, "tests", "golden", "make_icp_plane_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    d = mk.compute()  # asserts the decision margins >= 1e-9 itself
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_plane_golden.npz"))
    assert sorted(g.files) == sorted(d)
    assert g["target_normals"].dtype == np.float64 and np.array_equal(g["target_normals"], d["target_normals"])
    assert np.isfinite(g["target_normals"]).all()
    for kernel in ("l2", "tukey"):
        assert int(g[kernel + "_iterations"]) == int(d[kernel + "_iterations"])
        assert np.array_equal(g[kernel + "_correspondence_set"], d[kernel + "_correspondence_set"])
        assert np.linalg.norm(g[kernel + "_transformation"] - d[kernel + "_transformation"]) < 1e-12
        for k in ("_fitness", "_inlier_rmse", "_k"):
            assert abs(float(g[kernel + k]) - float(d[kernel + k])) <= 1e-12 * abs(float(d[kernel + k])), kernel + k
        assert (g[kernel + "_margins"] >= 1e-9).all()
        assert float(g[kernel + "_fitness"]) > float(g["init_fitness"])
    assert int(g["l2_iterations"]) < 19  # fewer than point-to-point needs on this pair (tests/golden/icp_golden.npz)


def test_public_names_defaults_and_value_errors():
    for name in ("TransformationEstimationPointToPlane", "L2Loss", "HuberLoss", "CauchyLoss", "GMLoss", "TukeyLoss"):
        assert name in tp.__all__ and hasattr(tp, name), name
    assert isinstance(tp.TransformationEstimationPointToPlane().kernel, tp.L2Loss)
    assert tp.TukeyLoss(0.1).k == 0.1 and tp.HuberLoss().k == 1.0
    assert [c.code for c in (tp.L2Loss, tp.HuberLoss, tp.CauchyLoss, tp.GMLoss, tp.TukeyLoss)] == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        tp.TransformationEstimationPointToPlane(kernel="tukey")
    sig = inspect.signature(tp.registration_icp)
    assert list(sig.parameters)[:7] == ["source", "target", "max_correspondence_distance", "init",
                                        "estimation_method", "criteria", "device"]
    assert sig.parameters["target_normals"].kind is inspect.Parameter.KEYWORD_ONLY
    bsig = inspect.signature(tp.registration_icp_batch).parameters
    assert bsig["estimation_methods"].default is None and bsig["target_normals"].default is None
    e = tp.icp.IcpEstimationC(7, 7, 7.0)
    assert tp.lib().teaser_hip_icp_estimation_default(e) == 0 and (e.method, e.kernel, e.kernel_k) == (0, 0, 1.0)
    assert tp.lib().teaser_hip_icp_estimation_default(None) == 1
    # refused before any library call (no device is needed to get these)
    P = np.zeros((5, 3))
    plane = tp.TransformationEstimationPointToPlane(tp.TukeyLoss(0.1))
    with pytest.raises(ValueError, match="target_normals"):
        tp.registration_icp(P, P, 0.1, np.eye(4), plane)
    with pytest.raises(ValueError, match="shape"):
        tp.registration_icp(P, P, 0.1, np.eye(4), plane, target_normals=np.zeros((4, 3)))
    with pytest.raises(ValueError, match="target_normals"):
        tp.registration_icp_batch([P, P], [P, P], 0.1, estimation_methods=[None, plane], target_normals=[None, None])
    with pytest.raises(ValueError):
        tp.registration_icp(P, P, 0.1, np.eye(4), "point-to-plane")
    with pytest.raises(ValueError):
        tp.registration_icp_batch([P], [P], 0.1, estimation_methods=[plane, plane], target_normals=[P])


def test_header_declares_and_library_exports_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "teaser_hip.h")).read()
    L = tp.lib()
    for name in ("teaser_hip_icp_estimation_default", "teaser_hip_icp_batch_ex", "teaser_hip_icp_solve_ex"):
        assert re.search(r"TEASER_HIP_API int32_t %s\(" % name, text), name
        assert name in tp.EXPORTED_SYMBOLS and getattr(L, name) is not None
    assert "typedef struct teaser_icp_estimation_c" in text
    assert C.sizeof(tp.icp.IcpEstimationC) == 16
    assert C.sizeof(tp.icp.IcpParamsC) == 32 and C.sizeof(tp.icp.IcpResultC) == 152  # layouts unchanged
    assert L.teaser_hip_abi_version() == 1


def test_plane_calls_use_the_ex_entry_and_point_calls_the_original(monkeypatch):
    calls = []

    class FakeLib:
        def teaser_hip_icp_create(self, device, out):
            out._obj.value = 4096
            return 0

        def teaser_hip_icp_batch(self, *a):
            calls.append(("batch", len(a)))
            return 0

        def teaser_hip_icp_batch_ex(self, *a):
            calls.append(("batch_ex", len(a), [(e.method, e.kernel, e.kernel_k) for e in a[-1]]))
            return 0

        def teaser_hip_icp_last_error(self, h):
            return b""

        def teaser_hip_icp_destroy(self, h):
            return 0

    monkeypatch.setattr(tp, "lib", lambda: FakeLib())
    monkeypatch.setattr(tp.icp._cache, "handles", {})
    monkeypatch.setattr(tp._handles, "_current_device", lambda: 0)
    P = np.zeros((4, 3))
    tp.registration_icp(P, P, 0.1)
    tp.registration_icp(P, P, 0.1, estimation_method=tp.TransformationEstimationPointToPoint())
    tp.registration_icp_batch([P, P], [P, P], 0.1, target_normals=[P, None],
                              estimation_methods=[tp.TransformationEstimationPointToPlane(tp.GMLoss(0.5)), None])
    assert calls == [("batch", 10), ("batch", 10), ("batch_ex", 12, [(1, 3, 0.5), (0, 0, 1.0)])]


def test_cxx_icp_plane_example_exits_77_without_device():
    from icp_plane_cxx import build_icp_plane_example
    exe = build_icp_plane_example()
    rc = subprocess.call([exe], stdout=subprocess.DEVNULL, timeout=120)
    assert rc == (0 if tp.device_count() > 0 else 77)
