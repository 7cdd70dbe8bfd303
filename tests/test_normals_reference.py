"""The numpy restatement of the normals contract (tests/normals_reference.py) against what is already pinned, and the
parts of the Python interface that need no GPU."""
import importlib
import os

import numpy as np
import pytest

import icp_gicp_reference as RG
import icp_reference as R
import normals_reference as RN
from util import ROOT

tp = importlib.import_module("teaser-plusplus_amd")


@pytest.fixture(scope="module")
def config5_target():
    _, Q, _, _ = R.config5_problem()
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_gicp_golden.npz"))
    radius, max_nn, eps = float(g["radius"]), int(g["max_nn"]), float(g["epsilon"])
    return Q, radius, max_nn, eps, RN.estimate_normals(Q, RN.HYBRID, radius, max_nn)


def test_normal_reproduces_the_pinned_covariances_on_the_config5_target(config5_target):
    Q, radius, max_nn, eps, (N, Cv, E, M) = config5_target
    ref = RG.estimate_covariances(Q, radius, max_nn, eps)
    got = np.tile(np.eye(3), (len(Q), 1, 1))
    for i in np.nonzero(M >= 3)[0]:
        got[i] = RG.covariance_from_unit_normal(N[i], eps)
    assert got.tobytes() == ref.tobytes()
    assert (M >= 3).sum() > 0.9 * len(Q)
    assert (np.diff(E, axis=1) >= 0).all() and np.array_equal(Cv, Cv.transpose(0, 2, 1))
    assert np.array_equal(N[M < 3], np.tile([[0.0, 0.0, 1.0]], ((M < 3).sum(), 1)))  # orient 0 fills (0, 0, 1)


def test_shuffled_summation_order_stays_inside_the_bar_on_the_test_clouds(config5_target):
    """The GPU test excludes the points whose bar 512 2^-52 lambda2 / (lambda1 - lambda0) exceeds 1e-6 and asserts that
    they are at most 1 % of a cloud; here the restatement against itself in a shuffled summation order stays inside
    the bar on the others, on the clouds that test uses."""
    Q, radius, max_nn, _, base = config5_target
    rng = np.random.default_rng(8)
    clouds = [(Q[::9], RN.HYBRID, 3 * radius, max_nn, RN.estimate_normals(Q[::9], RN.HYBRID, 3 * radius, max_nn)),
              (RN.cube(513), RN.KNN, 0.0, 33, RN.estimate_normals(RN.cube(513), RN.KNN, 0.0, 33))]
    for X, search, r, k, (N, _, E, M) in clouds:
        N2 = RN.estimate_normals(X, search, r, k, order=lambda js: rng.permutation(js))[0]
        bar = RN.normal_bar(E)
        use = (M >= 3) & (bar <= 1e-6)
        assert (~use & (M >= 3)).sum() <= 0.01 * len(X)
        err = np.minimum(np.linalg.norm(N2 - N, axis=1), np.linalg.norm(N2 + N, axis=1))
        assert (err[use] <= bar[use]).all()
    bar = RN.normal_bar(base[2])
    assert ((base[3] >= 3) & ~(bar <= 1e-6)).sum() <= 0.01 * len(Q)


def test_plane_gives_the_z_axis_and_a_zero_eigenvalue():
    X = RN.planar()
    for search, r in ((RN.HYBRID, 0.35), (RN.KNN, 0.0)):
        N, Cv, E, M = RN.estimate_normals(X, search, r, 12)
        assert (M >= 3).all()
        assert np.array_equal(np.abs(N), np.tile([[0.0, 0.0, 1.0]], (len(X), 1)))
        assert (E[:, 0] == 0).all() and (E[:, 1] > 0).all()
        assert (RN.surface_variation(E) == 0).all() and np.array_equal(tp.surface_variation(E), RN.surface_variation(E))


def test_orientation_flips_exactly_the_rows_with_a_negative_dot_product():
    X = RN.cube(129)
    N0, Cv0, E0, _ = RN.estimate_normals(X, RN.KNN, 0.0, 10)
    ref = np.array([0.5, 0.5, 3.0])
    N1 = RN.estimate_normals(X, RN.KNN, 0.0, 10, 1, ref)[0]
    N2 = RN.estimate_normals(X, RN.KNN, 0.0, 10, 2, ref)[0]
    V = ref - X
    d1 = (N0[:, 0] * V[:, 0] + N0[:, 1] * V[:, 1]) + N0[:, 2] * V[:, 2]
    d2 = (N0[:, 0] * ref[0] + N0[:, 1] * ref[1]) + N0[:, 2] * ref[2]
    assert (d1 < 0).any() and (d1 > 0).any()
    assert np.array_equal(N1, np.where((d1 < 0)[:, None], -N0, N0))
    assert np.array_equal(N2, np.where((d2 < 0)[:, None], -N0, N0))


def test_zero_normals_are_filled_in_by_the_three_rules():
    X = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [10.0, 3.0, 4.0]])  # nobody has three neighbours inside 1
    ref = np.array([10.0, 0.0, 0.0])
    N, Cv, E, M = RN.estimate_normals(X, RN.HYBRID, 1.0, 30)
    assert (M == 1).all() and not Cv.any() and not E.any()
    assert np.array_equal(N, np.tile([[0.0, 0.0, 1.0]], (3, 1)))
    N1 = RN.estimate_normals(X, RN.HYBRID, 1.0, 30, 1, ref)[0]
    assert np.array_equal(N1, [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -0.6, -0.8]])
    N2 = RN.estimate_normals(X, RN.HYBRID, 1.0, 30, 2, ref)[0]
    assert np.array_equal(N2, np.tile(ref, (3, 1)))
    for n in (1, 2):  # k-NN search below three points
        assert np.array_equal(RN.estimate_normals(RN.cube(n), RN.KNN, 0.0, 30)[0], np.tile([[0.0, 0.0, 1.0]], (n, 1)))


def test_python_interface_without_a_gpu():
    assert {"KDTreeSearchParamHybrid", "KDTreeSearchParamKNN", "estimate_normals", "estimate_normals_batch",
            "surface_variation"} <= set(tp.__all__)
    assert {"teaser_hip_icp_normals_batch", "teaser_hip_icp_batch_auto", "teaser_hip_icp_solve_auto"} <= set(
        tp.EXPORTED_SYMBOLS)
    sp = tp.KDTreeSearchParamHybrid(0.1, 30)
    al = sp.along([0, 0, 1])
    assert sp.orient == 0 and al.orient == 2 and al.ref == (0.0, 0.0, 1.0) and al.radius == 0.1 and al.max_nn == 30
    rec = tp.KDTreeSearchParamKNN().towards([1, 2, 3]).record()
    assert (rec.search, rec.max_nn, rec.orient, rec.reserved, list(rec.ref)) == (1, 30, 1, 0, [1.0, 2.0, 3.0])
    for bad in (lambda: tp.KDTreeSearchParamHybrid(0.1, 2), lambda: tp.KDTreeSearchParamKNN(101),
                lambda: tp.KDTreeSearchParamHybrid(0.0, 30), lambda: sp.along([0, np.nan, 1]),
                lambda: tp.estimate_normals(np.zeros((4, 3)), 0.1),
                lambda: tp.estimate_normals(np.zeros((4, 3)), sp, towards=[0, 0, 0], along=[0, 0, 1])):
        with pytest.raises(ValueError):
            bad()
    assert np.array_equal(tp.surface_variation([[1.0, 1.0, 2.0], [0.0, 0.0, 0.0]]), [0.25, 0.0])
    assert tp.estimate_normals_batch([], sp) == []
