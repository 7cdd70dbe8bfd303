"""The numpy restatement of the information matrices (tests/information_reference.py) against what it restates:
Open3D's GetInformationMatrixFromPointClouds builds, per correspondence with target point (x, y, z), the three rows
(0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1) and adds their outer products; the sum is the Hessian of
SUM |w x q + v|^2 in (w, v), checked here by finite differences.  No GPU."""
import numpy as np

import icp_reference as R
import information_reference as I


def pair(seed=5, n=60):
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-1, 1, size=(n, 3))
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.005]
    P = Q[: n - 10] + rng.normal(0, 0.002, size=(n - 10, 3)) - T[:3, 3]
    return P, Q, T


def test_rows_are_open3d_rows_and_the_sum_is_their_outer_products():
    P, Q, T = pair()
    ref = I.information(P, Q, 0.05, T)
    cs = ref["correspondence_set"]
    assert len(cs) > 30
    want = np.zeros((6, 6))
    for _, j in cs:
        x, y, z = Q[j]
        for row in ((0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0), (y, -x, 0, 0, 0, 1)):
            want += np.outer(row, row)
    assert np.allclose(ref["information"], want, rtol=1e-13, atol=0)
    assert ref["information"][5, 5] == len(cs) and np.array_equal(ref["information"][3:, 3:], len(cs) * np.eye(3))
    assert np.array_equal(ref["information"], ref["information"].T)
    vec, mag = I.information_vectorised(Q, cs[:, 1])
    assert np.allclose(vec, ref["information"], rtol=1e-13, atol=1e-13) and np.allclose(mag, ref["abs_terms"], rtol=1e-13)


def test_is_the_hessian_of_the_linearised_point_residual():
    """f(w, v) = 1/2 SUM_j |w x q_j + v|^2 has Hessian SUM G_j^T G_j: central second differences agree."""
    P, Q, T = pair(seed=9, n=40)
    ref = I.information(P, Q, 0.05, T)
    q = Q[ref["correspondence_set"][:, 1]]

    def f(u):
        return 0.5 * ((np.cross(u[:3], q) + u[3:]) ** 2).sum()

    h = 1e-3
    H = np.zeros((6, 6))
    E = np.eye(6) * h
    for a in range(6):
        for b in range(6):
            H[a, b] = (f(E[a] + E[b]) - f(E[a] - E[b]) - f(E[b] - E[a]) + f(-E[a] - E[b])) / (4 * h * h)
    assert np.allclose(H, ref["information"], rtol=1e-6, atol=1e-6)  # f is quadratic: only rounding separates them


def test_correspondences_are_the_icp_evaluation_and_empty_sets_give_zero():
    P, Q, T = pair()
    ref = I.information(P, Q, 0.05, T)
    icp = R.registration_icp(P, Q, 0.05, T, max_iteration=0)
    assert np.array_equal(ref["correspondence_set"], icp["correspondence_set"])
    assert ref["fitness"] == icp["fitness"] and ref["inlier_rmse"] == icp["inlier_rmse"]
    far = np.eye(4)
    far[:3, 3] = 50.0
    for args in ((P, Q, 0.05, far), (P[:0], Q, 0.05, T), (P, Q[:0], 0.05, T)):
        z = I.information(*args)
        assert not z["information"].any() and z["fitness"] == 0.0 and len(z["correspondence_set"]) == 0


def test_integer_grids_are_exact_in_both_types():
    rng = np.random.default_rng(3)
    Q = rng.integers(-64, 65, size=(300, 3)).astype(np.float64)
    P = Q[rng.permutation(300)[:200]]
    a = I.information(P, Q, 0.5, np.eye(4))
    b = I.information(P, Q, 0.5, np.eye(4), dtype=np.longdouble)
    assert a["information"][5, 5] == 200
    assert np.array_equal(a["information"].astype(np.longdouble), b["information"])
    vec, _ = I.information_vectorised(Q, a["correspondence_set"][:, 1])
    assert np.array_equal(vec, a["information"])


def test_python_front_ends_validate_and_fail_loudly_without_a_device():
    """The argument checks of the Python layer need no device; without one the calls raise NO_DEVICE (no CPU path)."""
    import importlib

    import pytest
    tp = importlib.import_module("teaser-plusplus_amd")
    P, Q, T = pair()
    with pytest.raises(ValueError, match="4 x 4"):
        tp.get_information_matrix_from_point_clouds(P, Q, 0.05, np.eye(3))
    with pytest.raises(ValueError, match="differ in length"):
        tp.get_information_matrix_from_point_clouds_batch([P, P], [Q], 0.05, T)
    with pytest.raises(ValueError, match="transformations"):
        tp.get_information_matrix_from_point_clouds_batch([P, P], [Q, Q], 0.05, np.zeros((3, 4, 4)))
    with pytest.raises(ValueError, match="n x 3"):
        tp.evaluate_registration(np.zeros((4, 2)), Q, 0.05)
    assert tp.get_information_matrix_from_point_clouds_batch([], [], 0.05, np.eye(4)).shape == (0, 6, 6)
    if tp.device_count() == 0:
        for call in (lambda: tp.get_information_matrix_from_point_clouds(P, Q, 0.05, T),
                     lambda: tp.evaluate_registration(P, Q, 0.05, T)):
            with pytest.raises(tp.TeaserHipError) as e:
                call()
            assert "NO_DEVICE" in str(e.value)


def test_cxx_information_example_compiles_and_exits_77_without_device():
    import importlib
    import subprocess

    from information_cxx import build_information_example
    tp = importlib.import_module("teaser-plusplus_amd")
    rc = subprocess.call([build_information_example()], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert rc == (0 if tp.device_count() > 0 else 77)
