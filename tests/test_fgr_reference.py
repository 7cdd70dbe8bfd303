"""The numpy restatement of Fast Global Registration (tests/fgr_reference.py) checked against what it restates: the
three rows are the derivative of the residual, the schedule, Open3D's ncorr < 10 rule, and the pose it recovers."""
import numpy as np
import pytest

import fgr_reference as ref


def test_rows_are_the_derivative_of_the_residual():
    """r(xi) = p - delta(xi) q; the rows J0, J1, J2 are dr/dxi at xi = 0 (central differences in longdouble)."""
    rng = np.random.default_rng(0)
    ld = np.longdouble
    for _ in range(5):
        p, q = rng.uniform(-1, 1, 3).astype(ld), rng.uniform(-1, 1, 3).astype(ld)
        J = ref.jacobian_rows(q)
        h = ld(1e-6)
        num = np.zeros((3, 6), dtype=ld)
        for k in range(6):
            xi = np.zeros(6, dtype=ld)
            xi[k] = h
            rp = p - ref.apply(ref.rotation(xi, ld), q[None, :])[0]
            rm = p - ref.apply(ref.rotation(-xi, ld), q[None, :])[0]
            num[:, k] = (rp - rm) / (2 * h)
        assert np.abs(num - J).max() < 1e-10  # truncation h^2 / 6 = 2e-13, rounding 1e-19 / h
    # and the 27 terms are s (sum J_k J_k^T) and s (sum e_k J_k)
    p, q = rng.uniform(-1, 1, (7, 3)), rng.uniform(-1, 1, (7, 3))
    v = ref.terms(p, q, 0.5)
    for c in range(7):
        J = ref.jacobian_rows(q[c])
        e = p[c] - q[c]
        s = (0.5 / (e @ e + 0.5)) ** 2
        A, g = ref.unpack(v[c])
        assert np.allclose(A, s * J.T @ J, rtol=1e-13, atol=1e-15)
        assert np.allclose(g, s * J.T @ e, rtol=1e-13, atol=1e-15)


def test_block_sum_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 255, 256, 257, 1025, 70000):
        x = rng.standard_normal((n, 2))
        got = ref.block_sum(x)
        assert np.allclose(got, x.sum(axis=0), rtol=0, atol=(n + 3) * 2.0 ** -52 * np.abs(x).sum(axis=0).max())
        assert np.array_equal(got, ref.block_sum(x))
    ints = np.arange(1, 601, dtype=np.float64)[:, None]  # exact in any order
    assert ref.block_sum(ints)[0] == 600 * 601 / 2


def test_mu_schedule_of_the_defaults_ends_at_1_4_to_the_minus_11():
    used, final = ref.mu_schedule(1.0, 64)
    assert len(used) == 64 and used[0] == 1.0 and used[1] == 1.0 / 1.4
    expect = 1.0
    for _ in range(11):
        expect = expect / 1.4
    assert final == expect and abs(final - 1.4 ** -11) < 1e-16
    assert len(set(used)) == 12 and used[-1] == final
    assert ref.mu_schedule(1.0, 64, decrease_mu=False) == ([1.0] * 64, 1.0)
    assert ref.mu_schedule(1.0, 64, maximum_correspondence_distance=0.6)[1] == 1.0 / 1.4 / 1.4


def test_fewer_than_ten_pairs_give_the_centroid_alignment():
    P, Q, corr, _ = ref.make_case(3, 40, 57, 9)
    out = ref.fgr(P, Q, corr)
    assert out["flags"] == 1 and out["iterations"] == 0 and len(out["mu"]) == 0
    T = out["transformation"]
    assert np.array_equal(T[:3, :3], np.eye(3))
    assert np.allclose(T[:3, 3], Q.mean(axis=0) - P.mean(axis=0), rtol=0, atol=1e-14)


def test_a_single_repeated_point_has_scale_zero():
    P, Q = np.full((5, 3), 0.5), np.full((12, 3), -1.25)
    corr = np.zeros((12, 2), dtype=np.int32)
    out = ref.fgr(P, Q, corr)
    assert out["flags"] == 2 and out["iterations"] == 0 and np.all(out["p"] == 0)
    assert np.allclose(out["transformation"][:3, 3], [-1.75] * 3)


@pytest.mark.parametrize("ncorr", [10, 64])
def test_clean_pairs_recover_the_pose(ncorr):
    P, Q, corr, T = ref.make_case(11, ncorr + 5, ncorr + 9, ncorr, outlier=0.0, noise=0.0, repeats=False)
    out = ref.fgr(P, Q, corr)
    assert out["failed_solves"] == 0 and out["iterations"] == 64
    assert np.abs(out["transformation"] - T).max() <= 1e-12


@pytest.mark.parametrize("ncorr,outlier", [(300, 0.3), (1025, 0.5), (2000, 0.8)])
def test_outliers_leave_the_pose_within_a_hundredth(ncorr, outlier):
    P, Q, corr, T = ref.make_case(12, ncorr + 50, ncorr + 80, ncorr, outlier=outlier, noise=1e-3, repeats=False)
    out = ref.fgr(P, Q, corr)
    assert np.abs(out["transformation"] - T).max() <= 1e-2


def test_stopping_after_n_steps_is_a_prefix_of_the_full_run():
    P, Q, corr, _, opt = ref.case("c65")
    full, part = ref.fgr(P, Q, corr, **opt), ref.fgr(P, Q, corr, n=7, **opt)
    assert np.array_equal(full["trans"][:7], part["trans"]) and np.array_equal(part["optimised"], full["trans"][6])
