"""The numpy restatement of the Open3D-form FPFH (tests/fpfh_o3d_reference.py) pinned without a GPU: (1) against a plain
scalar-loop transcription of the contract, bit for bit; (2) on hand-checked cases; (3) against the libm form of Open3D's
own expressions, which bounds how far the stated contract is from them."""
import importlib

import numpy as np
import pytest

import fpfh_o3d_reference as R

tp = importlib.import_module("teaser-plusplus_amd")


def both(P, N, search, radius, max_nn):
    idx, d2, m = R.neighbour_lists(P, search, radius, max_nn)
    H, _ = R.spfh_rows(P, N, idx, m)
    return (R.fpfh_rows(H, idx, d2, m), H), R.scalar_fpfh(P, N, idx, d2, m), m


# ---- part 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in R.case_list() if 0 < len(c[1]) <= 130])
def test_vectorised_restatement_equals_the_scalar_loops(name):
    _, P, N, search, radius, max_nn = next(c for c in R.case_list() if c[0] == name)
    (F, H), (Fs, Hs), _ = both(P, N, search, radius, max_nn)
    assert H.tobytes() == Hs.tobytes() and F.tobytes() == Fs.tobytes()


def test_deterministic_atan2_scalar_and_vector_forms_agree_and_are_close_to_libm():
    rng = np.random.default_rng(3)
    y, x = rng.normal(size=2000), rng.normal(size=2000)
    y[:6], x[:6] = [0.0, 0.0, 1.0, -1.0, 0.0, 2.0], [0.0, 1.0, 0.0, 0.0, -1.0, 2.0]
    a = R.det_atan2(y, x)
    assert all(a[k] == R.scalar_atan2(float(y[k]), float(x[k])) for k in range(len(y)))
    assert a[0] == 0.0 and a[1] == 0.0 and a[4] == R.PI
    assert np.abs(a - np.arctan2(y, x)).max() < 4 * 2.0 ** -52 * np.pi


# ---- part 2: hand-checked cases ------------------------------------------------------------------------------------------
def test_two_points_with_perpendicular_normals():
    """p1 = 0 with n1 = z, p2 = (1, 0, 0) with n2 = x.  From point 0: a1 = 0, a2 = 1, so the pair is swapped: n1 = x,
    n2 = z, dp = (-1, 0, 0), f2 = -1 -> bin 22.  v = dp x n1 = 0: degenerate after the swap, so all three features are 0:
    bins 5, 16, 27.  From point 1 (dp = (-1, 0, 0), n1 = x, n2 = z): |a1| = 1 > |a2| = 0, no swap, v = dp x n1 = 0:
    degenerate again.  m = 2: c = 100."""
    P = np.array([[0.0, 0, 0], [1, 0, 0]])
    N = np.array([[0.0, 0, 1], [1, 0, 0]])
    F, H = R.compute_fpfh_feature(P, N, R.KNN, 0.0, 2)
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(H[0], want) and np.array_equal(H[1], want)
    # a pair that is NOT degenerate: n1 = z at the origin, n2 = y at (1, 0, 0).  a1 = a2 = 0: no swap, f2 = 0 (bin 27);
    # v = dp x n1 = (0, -1, 0), w = n1 x v = (1, 0, 0); f1 = v . n2 = -1 (bin 11); f0 = atan2(w . n2, n1 . n2) =
    # atan2(0, 0) = 0 (bin 5)
    N2 = np.array([[0.0, 0, 1], [0, 1, 0]])
    f0, f1, f2, deg, sw = R.pair_features(P[0], N2[0], P[1], N2[1])
    assert (f0, f1, f2, bool(deg), bool(sw)) == (0.0, -1.0, 0.0, False, False)
    assert [int(h) for h in R.bins(f0, f1, f2)] == [5, 11, 27]
    # n2 = (0, 1, 1) / sqrt 2 turns f0 to atan2(0, cos 45) = 0 and f1 to -cos 45 -> floor(11 (1 - 0.7071) / 2) = 1
    n2 = np.array([0.0, 1, 1]) / np.sqrt(2.0)
    f0, f1, f2, _, _ = R.pair_features(P[0], N2[0], P[1], n2)
    assert [int(h) for h in R.bins(f0, f1, f2)] == [5, 12, 27]
    # FPFH of point 0: one neighbour at d2 = 1: F = H[1] / 1, S = 100 per group, F = F 100 / 100 + H[0]
    assert np.array_equal(F[0], 100.0 * H[1] / 100.0 + H[0]) and F[0, 5] == 200.0


def test_dp_parallel_to_n1_is_degenerate_and_lands_in_bins_5_16_27():
    f = R.pair_features(np.zeros(3), np.array([0.0, 0, 1]), np.array([0.0, 0, 2]), np.array([0.0, 1, 0]))
    assert f[0] == 0 and f[1] == 0 and f[2] == 0 and bool(f[3])
    assert [int(h) for h in R.bins(f[0], f[1], f[2])] == [5, 16, 27]
    assert R.scalar_pair([0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 1, 0]) == (0.0, 0.0, 0.0)


def test_coincident_points():
    """Every pair has f3 = 0: SPFH is 100 in bins 5, 16 and 27, and FPFH equals SPFH because every d2 == 0 is skipped."""
    P = np.tile([[0.3, -1.25, 7.0]], (9, 1))
    _, N = R.random_cloud(9, 2)
    for search, k in ((R.HYBRID, 5), (R.KNN, 9)):
        (F, H), (Fs, Hs), m = both(P, N, search, 0.5, k)
        want = np.zeros(33)
        want[[5, 16, 27]] = 100.0
        assert (m == k).all() and all(np.array_equal(h, want) for h in H)
        assert np.array_equal(F, H) and np.array_equal(Fs, Hs) and np.array_equal(F, Fs)
    # position 0 is skipped by position: the list of point 3 begins with index 0, and the point meets itself at k = 3
    idx, _, _ = R.neighbour_lists(P, R.KNN, 0.0, 9)
    assert idx[3, 0] == 0 and idx[3, 3] == 3


def test_rows_with_one_neighbour_are_zero():
    P, N = R.random_cloud(12, 4)
    (F, H), (Fs, Hs), m = both(P, N, R.HYBRID, 1e-3, 10)
    assert (m == 1).all() and not F.any() and not H.any() and not Fs.any() and not Hs.any()
    F1, H1 = R.compute_fpfh_feature(P[:1], N[:1], R.KNN, 0.0, 5)
    assert F1.shape == (1, 33) and not F1.any() and not H1.any()
    assert R.compute_fpfh_feature(np.zeros((0, 3)), np.zeros((0, 3)), R.KNN, 0.0, 5)[0].shape == (0, 33)


def test_equal_cosines_do_not_swap():
    """n1 = n2 = (1, 0, 1) / sqrt 2 and dp along x: a1 == a2 exactly; f2 = a1, the normals stay where they are."""
    n = np.array([1.0, 0, 1]) / np.sqrt(2.0)
    p2 = np.array([1.0, 0, 0])
    f0, f1, f2, deg, sw = R.pair_features(np.zeros(3), n, p2, n)
    assert not bool(sw) and not bool(deg) and f2 == n[0]
    # the strict comparison decides: nudging a2 up by one ulp swaps, and f2 changes sign
    n2 = np.array([np.nextafter(n[0], 1.0), 0.0, n[2]])
    g = R.pair_features(np.zeros(3), n, p2, n2)
    assert bool(g[4]) and g[2] == -n2[0]
    # the lattice of the shared cases holds such ties
    P, N = R.axis_lattice(4)
    idx, _, m = R.neighbour_lists(P, R.KNN, 0.0, 27)
    i = np.repeat(np.arange(len(P)), 26)
    j = idx[:, 1:27].ravel()
    dp = P[j] - P[i]
    f3 = np.sqrt(R.dot(dp, dp))
    a1, a2 = R.dot(N[i], dp) / f3, R.dot(N[j], dp) / f3
    _, _, _, deg, sw = R.pair_features(P[i], N[i], P[j], N[j])
    tie = np.abs(a1) == np.abs(a2)
    assert tie.sum() > 100 and not sw[tie].any() and deg.sum() > 10


# ---- part 3: the stated contract against Open3D's own expressions (libm) ----------------------------------------------------
def generic_clouds():
    rng = np.random.default_rng(7)
    s = R.unit(rng.normal(size=(1500, 3)))
    sphere = s * (1.0 + 0.01 * rng.normal(size=(1500, 1)))
    plane = np.concatenate([rng.random((1500, 2)) * 2.0, 0.01 * rng.normal(size=(1500, 1))], 1)
    pn = R.unit(np.array([0.0, 0, 1]) + 0.05 * rng.normal(size=(1500, 3)))
    return [("noisy unit sphere", sphere, R.unit(s + 0.05 * rng.normal(size=(1500, 3)))), ("noisy plane", plane, pn)]


def test_restatement_against_the_libm_form_on_two_generic_clouds():
    """np.arctan2 for f0 and Open3D's own swap test acos(|a1|) > acos(|a2|), against the deterministic atan2 and the
    comparison of the cosines: at most 1 neighbour pair in 10 000 may fall into a different bin triple.
    Measured here (default_rng(7), 1 500 points each, hybrid 0.25 / 100): noisy unit sphere 35 028 pairs, noisy plane
    97 674 pairs, 132 702 in all: 0 pairs in a different bin triple, 0 different swap decisions."""
    libm_swap = lambda a1, a2: np.arccos(np.minimum(np.abs(a1), 1.0)) > np.arccos(np.minimum(np.abs(a2), 1.0))  # noqa: E731
    pairs = differ = swaps = 0
    for name, P, N in generic_clouds():
        idx, _, m = R.neighbour_lists(P, R.HYBRID, 0.25, 100)
        _, ours = R.spfh_rows(P, N, idx, m)
        _, libm = R.spfh_rows(P, N, idx, m, atan2=np.arctan2, swap=libm_swap)
        i = np.repeat(np.arange(len(P)), np.maximum(m - 1, 0))
        j = np.concatenate([idx[r, 1:m[r]] for r in range(len(P))])
        sw_ours = R.pair_features(P[i], N[i], P[j], N[j])[4]
        sw_libm = R.pair_features(P[i], N[i], P[j], N[j], np.arctan2, libm_swap)[4]
        assert len(ours) == len(libm) == len(i) == int(np.maximum(m - 1, 0).sum())
        d = int((ours != libm).any(axis=1).sum())
        s = int((sw_ours != sw_libm).sum())
        print("%s: %d pairs, %d in a different bin triple, %d swap decisions differ" % (name, len(ours), d, s))
        pairs, differ, swaps = pairs + len(ours), differ + d, swaps + s
    assert pairs > 100000
    assert differ * 10000 <= pairs


# ---- the Python layer's checks that need no device ------------------------------------------------------------------------
def test_python_layer_refuses_before_it_reaches_the_device():
    P, N = R.random_cloud(8, 1)
    for name in ("compute_fpfh_feature", "compute_fpfh_feature_batch", "extract_fpfh", "KDTreeSearchParamRadius"):
        assert name in tp.__all__ and hasattr(tp, name), name
    with pytest.raises(ValueError, match="KDTreeSearchParamRadius"):
        tp.compute_fpfh_feature(P, N, tp.KDTreeSearchParamRadius(0.3))
    with pytest.raises(ValueError, match="orient"):
        tp.compute_fpfh_feature(P, N, tp.KDTreeSearchParamKNN(5).along([0, 0, 1]))
    with pytest.raises(ValueError, match="8 points and 7 normals"):
        tp.compute_fpfh_feature(P, N[:7], tp.KDTreeSearchParamKNN(5))
    with pytest.raises(ValueError, match="non-finite"):
        tp.compute_fpfh_feature(P, np.where(np.arange(24).reshape(8, 3) == 5, np.inf, N), tp.KDTreeSearchParamKNN(5))
    with pytest.raises(ValueError, match="neither normals"):
        tp.compute_fpfh_feature_batch([P], [None], tp.KDTreeSearchParamKNN(5))
    with pytest.raises(ValueError, match="max_nn"):
        tp.compute_fpfh_feature(P, N, ("knn", 101))
