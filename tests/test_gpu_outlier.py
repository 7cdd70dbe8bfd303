"""Self k-NN, statistical and radius outlier removal on the MI355X against the numpy restatement of the contract
(tests/outlier_reference.py): indices, d2 bits, avg bits, stats bits, counts and masks are EQUAL -- nothing in the
contract depends on an order of evaluation that is left open, so there is no tolerance.  (One exception, stated in
outlier_reference.bits_equal: a NaN equals a NaN whatever its sign bit; std = sqrt(0 / 0) for n = 1 is the only one.)
Shapes: the smallest at which each path is taken -- both list capacities (k <= 32 and k > 32), one and several blocks of
64 and of 256 points, k below, at and above n, the ring route, the whole-cloud route and a cloud that needs both."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import outlier_reference as R
from util import ROOT

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def check_knn(P, k, got=None):
    idx, d2 = got if got is not None else tp.self_knn(P, k, return_distance=True)
    ridx, rd2 = R.self_knn(P, k)
    assert idx.shape == ridx.shape and idx.dtype == np.int32
    bad = np.flatnonzero((idx != ridx).any(axis=1))
    assert len(bad) == 0, "k = %d: %d rows differ, first %d: %s vs %s" % (k, len(bad), bad[0], idx[bad[0]], ridx[bad[0]])
    assert R.bits_equal(d2, rd2)


def check_statistical(P, nb, ratio, got=None):
    pts, ind, st = got if got is not None else tp.remove_statistical_outlier(P, nb, ratio, return_stats=True)
    ref = R.statistical(P, nb, ratio)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    assert R.bits_equal(st["avg"], ref["avg"])
    if len(P):
        assert R.bits_equal([st["mean"], st["std"], st["threshold"]], [ref["mean"], ref["std"], ref["threshold"]])
    assert np.array_equal(ind, np.flatnonzero(ref["keep"])) and np.array_equal(pts, P[ind])
    return ref


def check_radius(P, nb, r, got=None):
    pts, ind, cnt = got if got is not None else tp.remove_radius_outlier(P, nb, r, return_counts=True)
    ref = R.radius(P, nb, r)
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(cnt, ref["count"]) and np.array_equal(ind, np.flatnonzero(ref["keep"]))
    assert np.array_equal(pts, P[ind])
    return ref


def lattice(m=7, h=0.125):
    g = h * np.arange(m)
    return np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], 1)


def test_lattice_ties_go_to_the_smaller_index_and_permute_with_the_cloud():
    P = lattice()  # 343 points, dyadic spacing: massive exact d2 ties
    ks = [1, 2, 7, 27, 100]
    got = tp.self_knn_batch([P] * len(ks), ks, return_distance=True)
    for k, g in zip(ks, got):
        check_knn(P, k, g)
    perm = np.random.default_rng(3).permutation(len(P))
    Q = P[perm]
    for k, g in zip(ks, tp.self_knn_batch([Q] * len(ks), ks, return_distance=True)):
        check_knn(Q, k, g)
        # point i of Q is point perm[i] of P: the same distances in the same order (the indices are Q's own, and a
        # tie class cut by k keeps its smallest indices in Q's numbering, which check_knn has just verified)
        assert R.bits_equal(g[1], got[ks.index(k)][1][perm])
    check_statistical(P, 7, 1.0)
    check_statistical(Q, 27, 0.5)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 513])
def test_block_edge_sizes_with_k_below_at_and_above_n(n):
    rng = np.random.default_rng(100 + n)
    P = rng.random((n, 3))
    ks = sorted({k for k in (1, n - 1, n, n + 1, 33, 100) if 1 <= k <= 100})
    empty = np.zeros((0, 3))
    clouds = []
    for k in ks:
        clouds += [P, empty]  # an empty cloud in the middle of the batch, every time
    kk = [k for k in ks for _ in (0, 1)]
    got = tp.self_knn_batch(clouds, kk, return_distance=True)
    for c, (k, g) in enumerate(zip(kk, got)):
        if c % 2:
            assert g[0].shape == (0, k) and g[1].shape == (0, k)
        else:
            check_knn(P, k, g)
    res = tp.remove_statistical_outlier_batch(clouds, kk, 1.5, return_stats=True)
    for c, (k, g) in enumerate(zip(kk, res)):
        if c % 2:
            assert len(g[1]) == 0 and np.isnan(g[2]["threshold"])
        else:
            check_statistical(P, k, 1.5, g)
    rad = tp.remove_radius_outlier_batch([P, empty, P], [1, 3, 4], [0.2, 0.1, 0.35], return_counts=True)
    check_radius(P, 1, 0.2, rad[0])
    assert len(rad[1][1]) == 0
    check_radius(P, 4, 0.35, rad[2])


def test_degenerate_clouds():
    rng = np.random.default_rng(8)
    same = np.tile([[0.3, -1.25, 7.0]], (300, 1))
    t = rng.random(400)
    line = np.outer(t, [1.0, 2.0, -0.5]) + [3.0, 0.0, 1.0]
    plane = np.stack([rng.random(500), rng.random(500), np.full(500, 0.75)], 1)
    axis_line = np.stack([np.zeros(200), rng.random(200), np.zeros(200)], 1)
    for P in (same, line, plane, axis_line):
        for k in (5, 40):
            check_knn(P, k)
        check_statistical(P, 20, 2.0)
        check_radius(P, 3, 0.05)
    assert len(tp.remove_statistical_outlier(same, 20, 2.0)[1]) == 0  # every avg is 0
    # 40 exact copies of one point, 20 neighbours: their avg is 0 and they are dropped (the avg > 0 rule)
    dup = rng.random((500, 3))
    copies = rng.choice(500, size=40, replace=False)
    dup[copies] = dup[copies[0]]
    ref = check_statistical(dup, 20, 2.0)
    assert (ref["avg"][copies] == 0).all() and not ref["keep"][copies].any() and ref["keep"].sum() > 300
    check_knn(dup, 20)


def far_cloud():
    rng = np.random.default_rng(17)
    P = rng.random((2002, 3))
    P[700] = 1000.0 * np.ones(3)   # 1 000 x the extent
    P[1300] = 1.0e6 * np.ones(3)   # 10^6 x the extent
    return P


def test_far_outliers_take_the_fallback_and_the_route_never_shows():
    P = far_cloud()
    assert tp.get_icp_option("knn_ring_cap") == 4
    a = tp.self_knn(P, 20, return_distance=True)
    fell = tp.get_icp_option("knn_fallbacks")
    assert 1 <= fell < len(P), fell
    check_knn(P, 20, a)
    s = tp.remove_statistical_outlier(P, 20, 2.0, return_stats=True)
    assert tp.get_icp_option("knn_fallbacks") >= 1
    check_statistical(P, 20, 2.0, s)
    assert 1300 not in s[1]
    try:
        tp.set_icp_option("knn_ring_cap", 0)  # every query through the whole-cloud scan
        b = tp.self_knn(P, 20, return_distance=True)
        assert tp.get_icp_option("knn_fallbacks") == len(P)
        s0 = tp.remove_statistical_outlier(P, 20, 2.0, return_stats=True)
        assert tp.get_icp_option("knn_fallbacks") == len(P)
        c = tp.self_knn(P, 100, return_distance=True)  # the long-list instantiation of the scan
    finally:
        tp.set_icp_option("knn_ring_cap", 4)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(s[1], s0[1]) and s[2]["avg"].tobytes() == s0[2]["avg"].tobytes()
    assert [s[2][key] for key in ("mean", "std", "threshold")] == [s0[2][key] for key in ("mean", "std", "threshold")]
    d = tp.self_knn(P, 100, return_distance=True)
    assert np.array_equal(c[0], d[0]) and c[1].tobytes() == d[1].tobytes()
    with pytest.raises(tp.TeaserHipError, match="knn_ring_cap"):
        tp.set_icp_option("knn_ring_cap", 17)
    with pytest.raises(tp.TeaserHipError, match="read-only"):
        tp.set_icp_option("knn_fallbacks", 0)
    with pytest.raises(tp.TeaserHipError, match="no_such_option"):
        tp.get_icp_option("no_such_option")


@pytest.mark.parametrize("shift,scale", [(1.0e4, 1.0), (0.0, 1.0e-3), (-1.0e4, 1.0e-3)])
def test_far_from_the_origin_and_tiny_coordinates(shift, scale):
    P = np.random.default_rng(23).random((1000, 3)) * scale + shift
    check_knn(P, 20)
    check_knn(P, 64)
    check_statistical(P, 20, 2.0)
    check_radius(P, 5, 0.1 * scale)


def test_radius_is_strict_and_bucket_collisions_count_once():
    P = lattice(5, 0.25)
    ref = check_radius(P, 1, 0.25)  # the lattice neighbours sit at exactly the radius: excluded
    assert (ref["count"] == 1).all()
    r = 0.25 * np.sqrt(2.0) * 1.0000001  # axis and face-diagonal neighbours inside
    cnt = R.radius(P, 1, r)["count"]
    c = int(cnt[62])  # the centre point of the lattice: 1 + 6 + 12
    assert c == 19
    for nb in (c - 1, c, c + 1):
        ref = check_radius(P, nb, r)
        assert bool(ref["keep"][62]) == (c > nb)
    # n = 5: the bucket table has 16 entries, so the 27 cell offsets reach the same buckets again and again
    five = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.15, 0.15, 0.1], [0.9, 0.9, 0.9]])
    for rr in (0.05, 0.12, 0.2, 0.26, 2.0):
        for nb in (1, 2, 4):
            check_radius(five, nb, rr)
    check_knn(five, 3)
    check_statistical(five, 3, 1.0)


def fresh_handle_covariances(P, radius, max_nn):
    """teaser_hip_icp_covariances_batch for one cloud on a newly created handle, destroyed afterwards."""
    L = tp.lib()
    h = C.c_void_p()
    assert L.teaser_hip_icp_create(0, C.byref(h)) == 0
    try:
        P = np.ascontiguousarray(P, dtype=np.float64)
        out = np.empty((len(P), 3, 3))
        rc = L.teaser_hip_icp_covariances_batch(
            h, 1, (_dp * 1)(P.ctypes.data_as(_dp)), np.array([len(P)], dtype=np.int32).ctypes.data_as(_ip),
            np.array([radius], dtype=np.float64).ctypes.data_as(_dp),
            np.array([max_nn], dtype=np.int32).ctypes.data_as(_ip), None, (_dp * 1)(out.ctypes.data_as(_dp)))
        assert rc == 0, L.teaser_hip_icp_last_error(h).decode()
        return out
    finally:
        L.teaser_hip_icp_destroy(h)


def test_mixed_batch_gives_each_cloud_its_own_bits_and_leaves_the_handle_clean():
    rng = np.random.default_rng(31)
    sizes = [0, 1, 3000, 40, 257, 0, 1200, 64, 700]
    clouds = [rng.random((n, 3)) * rng.uniform(0.5, 3.0, size=3) for n in sizes]
    clouds[6][5] = [50.0, 50.0, 50.0]
    ks = [5, 3, 20, 100, 33, 7, 64, 32, 1]
    ratios = [1.0, 2.0, 2.0, 0.5, 1.5, 1.0, 3.0, 0.7, 2.0]
    radii = [0.1, 0.1, 0.12, 0.6, 0.3, 0.1, 0.2, 0.5, 0.25]
    cov_in = clouds[2][:800]
    cov_ref = fresh_handle_covariances(cov_in, 0.3, 20)  # a handle no outlier call has ever touched
    knn = tp.self_knn_batch(clouds, ks, return_distance=True)
    st = tp.remove_statistical_outlier_batch(clouds, ks, ratios, return_stats=True)
    cov_mid = tp.estimate_covariances(cov_in, 0.3, 20)
    rad = tp.remove_radius_outlier_batch(clouds, [2] * 9, radii, return_counts=True)
    knn2 = tp.self_knn_batch(clouds, ks, return_distance=True)
    st2 = tp.remove_statistical_outlier_batch(clouds, ks, ratios, return_stats=True)
    rad2 = tp.remove_radius_outlier_batch(clouds, [2] * 9, radii, return_counts=True)
    cov_end = tp.estimate_covariances(cov_in, 0.3, 20)
    assert cov_ref.tobytes() == cov_mid.tobytes() == cov_end.tobytes()
    assert cov_ref.tobytes() == fresh_handle_covariances(cov_in, 0.3, 20).tobytes()
    assert not np.array_equal(cov_ref, np.tile(np.eye(3), (len(cov_in), 1, 1)))  # real normals, not all identity
    for c in range(9):
        P, k = clouds[c], ks[c]
        alone = tp.self_knn(P, k, return_distance=True)
        for g in (knn[c], knn2[c]):
            assert np.array_equal(g[0], alone[0]) and g[1].tobytes() == alone[1].tobytes()
        s1 = tp.remove_statistical_outlier(P, k, ratios[c], return_stats=True)
        for g in (st[c], st2[c]):
            assert np.array_equal(g[1], s1[1]) and g[2]["avg"].tobytes() == s1[2]["avg"].tobytes()
            assert R.bits_equal([g[2][key] for key in ("mean", "std", "threshold")],
                                [s1[2][key] for key in ("mean", "std", "threshold")])
        r1 = tp.remove_radius_outlier(P, 2, radii[c], return_counts=True)
        for g in (rad[c], rad2[c]):
            assert np.array_equal(g[1], r1[1]) and np.array_equal(g[2], r1[2])
        check_knn(P, k, alone)
        check_statistical(P, k, ratios[c], s1)
        check_radius(P, 2, radii[c], r1)


def test_config5_clouds_equal_the_restatement():
    d = np.load(os.path.join(ROOT, "tests", "golden", "config5_clouds.npz"))
    clouds = [d["cloud_bin_0"], d["cloud_bin_4"]]
    res = tp.remove_statistical_outlier_batch(clouds, 20, 2.0, return_stats=True)
    for P, g in zip(clouds, res):
        ref = check_statistical(P, 20, 2.0, g)
        print("config-5 cloud: %d points, %d kept, mean %.6g std %.6g" % (len(P), ref["keep"].sum(), ref["mean"], ref["std"]))
        assert 0 < ref["keep"].sum() < len(P)


def _c_handle():
    L = tp.lib()
    h = C.c_void_p()
    assert L.teaser_hip_icp_create(0, C.byref(h)) == 0
    return L, h


def test_invalid_arguments_are_refused_by_name_and_the_handle_survives():
    L, h = _c_handle()
    try:
        rng = np.random.default_rng(2)
        A, Bc = np.ascontiguousarray(rng.random((50, 3))), np.ascontiguousarray(rng.random((60, 3)))
        bad = Bc.copy()
        bad[7, 1] = np.nan
        n = np.array([50, 60], dtype=np.int32)

        def ptrs(*arrs):
            return (_dp * len(arrs))(*[a.ctypes.data_as(_dp) for a in arrs])

        keep = [np.zeros(50, dtype=np.uint8), np.zeros(60, dtype=np.uint8)]
        kp = (_bp * 2)(*[a.ctypes.data_as(_bp) for a in keep])
        kept = np.zeros(2, dtype=np.int32)
        idx = [np.zeros((50, 100), dtype=np.int32), np.zeros((60, 100), dtype=np.int32)]
        ip = (_ip * 2)(*[a.ctypes.data_as(_ip) for a in idx])
        i32 = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(_ip)  # noqa: E731
        f64 = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(_dp)  # noqa: E731
        np_ = n.ctypes.data_as(_ip)
        kq = kept.ctypes.data_as(_ip)

        def refused(rc, *words):
            msg = L.teaser_hip_icp_last_error(h).decode()
            assert rc == 1, (rc, msg)  # TEASER_HIP_ERR_BAD_ARG
            for w in words:
                assert w in msg, msg

        stat = L.teaser_hip_icp_remove_statistical_outliers_batch
        rad = L.teaser_hip_icp_remove_radius_outliers_batch
        knn = L.teaser_hip_icp_self_knn_batch
        refused(stat(h, 2, ptrs(A, bad), np_, i32(20, 20), f64(2, 2), kp, kq, None, None), "points", "non-finite", "problem 1")
        refused(stat(h, 2, ptrs(A, Bc), np_, i32(20, 0), f64(2, 2), kp, kq, None, None), "nb_neighbors", "problem 1")
        refused(stat(h, 2, ptrs(A, Bc), np_, i32(101, 20), f64(2, 2), kp, kq, None, None), "nb_neighbors", "problem 0")
        for r in (0.0, -1.0, np.inf, np.nan):
            refused(stat(h, 2, ptrs(A, Bc), np_, i32(20, 20), f64(2, r), kp, kq, None, None), "std_ratio", "problem 1")
        refused(stat(h, 2, (_dp * 2)(A.ctypes.data_as(_dp), None), np_, i32(20, 20), f64(2, 2), kp, kq, None, None),
                "points is NULL", "problem 1")
        refused(stat(h, 2, ptrs(A, Bc), np_, i32(20, 20), f64(2, 2), (_bp * 2)(keep[0].ctypes.data_as(_bp), None), kq,
                     None, None), "keep_out", "problem 1")
        refused(rad(h, 2, ptrs(A, bad), np_, i32(2, 2), f64(0.1, 0.1), kp, kq, None), "points", "problem 1")
        for r in (0.0, -0.5, np.inf, np.nan, 1e200, 1e-200):
            refused(rad(h, 2, ptrs(A, Bc), np_, i32(2, 2), f64(r, 0.1), kp, kq, None), "radius", "problem 0")
        refused(rad(h, 2, ptrs(A, Bc), np_, i32(2, 0), f64(0.1, 0.1), kp, kq, None), "nb_points", "problem 1")
        refused(rad(h, 2, ptrs(A, Bc), np_, i32(2, 2), f64(0.1, 0.1), None, kq, None), "keep_out", "problem 0")
        refused(knn(h, 2, ptrs(A, bad), np_, i32(5, 5), ip, None), "points", "problem 1")
        refused(knn(h, 2, ptrs(A, Bc), np_, i32(5, 101), ip, None), "k must lie", "problem 1")
        refused(knn(h, 2, ptrs(A, Bc), np_, i32(0, 5), ip, None), "k must lie", "problem 0")
        refused(knn(h, 2, ptrs(A, Bc), np_, i32(5, 5), None, None), "idx_out", "problem 0")
        # the handle works afterwards, and an empty cloud with NULL pointers is legal
        n0 = np.array([50, 0], dtype=np.int32)
        rc = stat(h, 2, (_dp * 2)(A.ctypes.data_as(_dp), None), n0.ctypes.data_as(_ip), i32(20, 20), f64(2, 2),
                  (_bp * 2)(keep[0].ctypes.data_as(_bp), None), kq, None, None)
        assert rc == 0, L.teaser_hip_icp_last_error(h).decode()
        ref = R.statistical(A, 20, 2.0)
        assert np.array_equal(keep[0], ref["keep"]) and kept.tolist() == [int(ref["keep"].sum()), 0]
    finally:
        L.teaser_hip_icp_destroy(h)


def test_cxx_facade_keeps_the_literal_index_set():
    import subprocess

    from outlier_cxx import build_outlier_example
    exe = build_outlier_example()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "checks 1" in out.stdout, out.stdout + out.stderr
