"""Pins tests/search_reference.py, the numpy restatement of the neighbour-search contract: against straight scalar
loops, against outlier_reference where query = data, the hybrid row as a prefix of the radius row, the strict
boundary, and the declarations of the three entry points.  No GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

import outlier_reference as R
import search_reference as S

tp = importlib.import_module("teaser-plusplus_amd")


def loop_rows(P, Q):
    """Per query the list of (d2, j) over the data in ascending order, by scalar arithmetic."""
    rows = []
    for q in Q:
        row = []
        for j, p in enumerate(P):
            dx, dy, dz = float(q[0]) - float(p[0]), float(q[1]) - float(p[1]), float(q[2]) - float(p[2])
            row.append(((dx * dx + dy * dy) + dz * dz, j))
        rows.append(sorted(row))
    return rows


def problems():
    rng = np.random.default_rng(17)
    P = rng.random((41, 3))
    return [(P, rng.random((23, 3)) * 1.5 - 0.25), (S.lattice(3), S.lattice_centres(3)), (S.lattice(3), S.lattice(3)),
            (P, np.zeros((0, 3))), (np.zeros((0, 3)), P[:5]), (np.tile([[1.0, 2.0, 3.0]], (9, 1)), P[:4] + 1.0)]


@pytest.mark.parametrize("case", range(6))
def test_restatement_equals_scalar_loops(case):
    P, Q = problems()[case]
    rows = loop_rows(P, Q)
    for k in (1, 5, 50):
        idx, d2 = S.knn_search(P, Q, k)
        assert idx.shape == (len(Q), k) and idx.dtype == np.int32
        for i, row in enumerate(rows):
            m = min(k, len(P))
            assert idx[i, :m].tolist() == [j for _, j in row[:m]] and (idx[i, m:] == -1).all()
            assert d2[i, :m].tolist() == [d for d, _ in row[:m]] and np.isinf(d2[i, m:]).all()
    for radius in (0.25, 0.4, 10.0):
        r2 = radius * radius
        idx, d2, splits = S.radius_search(P, Q, radius)
        assert splits.dtype == np.int64 and len(splits) == len(Q) + 1 and splits[-1] == len(idx) == len(d2)
        for i, row in enumerate(rows):
            inside = [(d, j) for d, j in row if d < r2]
            assert idx[splits[i]:splits[i + 1]].tolist() == [j for _, j in inside]
            assert d2[splits[i]:splits[i + 1]].tolist() == [d for d, _ in inside]
        for max_nn in (1, 4, 100):
            hidx, hd2, cnt = S.hybrid_search(P, Q, radius, max_nn)
            for i in range(len(Q)):  # the hybrid row is the prefix of the radius row
                m = min(max_nn, int(splits[i + 1] - splits[i]))
                assert cnt[i] == m
                assert np.array_equal(hidx[i, :m], idx[splits[i]:splits[i] + m]) and (hidx[i, m:] == -1).all()
                assert R.bits_equal(hd2[i, :m], d2[splits[i]:splits[i] + m]) and np.isinf(hd2[i, m:]).all()


def test_query_equal_to_data_is_self_knn_and_the_radius_count():
    rng = np.random.default_rng(5)
    for P in (rng.random((130, 3)), S.lattice(4)):
        for k in (1, 7, 33):
            idx, d2 = S.knn_search(P, P, k)
            ridx, rd2 = R.self_knn(P, k)
            assert np.array_equal(idx, ridx) and R.bits_equal(d2, rd2)
        for radius in (0.1, 0.25, 0.3):
            splits = S.radius_search(P, P, radius)[2]
            assert np.array_equal(np.diff(splits), R.radius(P, 1, radius)["count"])


def test_the_boundary_is_strict():
    P = S.lattice(4)
    idx, d2, splits = S.radius_search(P, P, 0.25)  # the six axis neighbours sit at exactly the radius: excluded
    assert np.array_equal(np.diff(splits), np.ones(len(P))) and np.array_equal(idx, np.arange(len(P)))
    assert (d2 == 0).all()
    hidx, _, cnt = S.hybrid_search(P, P, 0.25, 8)
    assert (cnt == 1).all() and np.array_equal(hidx[:, 0], np.arange(len(P))) and (hidx[:, 1:] == -1).all()
    inner = S.radius_search(P, P[21:22], 0.25 * 1.0001)  # an interior point: itself and its six neighbours
    assert len(inner[0]) == 7 and inner[0][0] == 21 and (inner[1][1:] == 0.0625).all()
    assert inner[0][1:].tolist() == sorted(inner[0][1:].tolist())
    # a cell centre: the eight corners tie and come in index order
    idx, d2 = S.knn_search(P, S.lattice_centres(4)[:1], 8)
    assert idx[0].tolist() == [0, 1, 4, 5, 16, 17, 20, 21] and (d2 == 3 * 0.125 ** 2).all()


def test_declarations_and_exports():
    L = type("L", (), {})()
    for name in ("knn", "hybrid", "radius"):
        setattr(L, "teaser_hip_icp_%s_search_batch" % name, type("F", (), {})())
    tp.search.declare(L)
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    head = [C.c_void_p, C.c_int32, C.POINTER(dp), ip, C.POINTER(dp), ip]
    assert L.teaser_hip_icp_knn_search_batch.argtypes == head + [ip, C.POINTER(ip), C.POINTER(dp)]
    assert L.teaser_hip_icp_hybrid_search_batch.argtypes == head + [dp, ip, C.POINTER(ip), C.POINTER(dp), C.POINTER(ip)]
    assert L.teaser_hip_icp_radius_search_batch.argtypes == head + [dp, lp, C.POINTER(ip), C.POINTER(ip), C.POINTER(dp),
                                                                    lp]
    assert [len(getattr(L, "teaser_hip_icp_%s_search_batch" % n).argtypes) for n in ("knn", "hybrid", "radius")] == \
        [9, 11, 12]
    for name in ("teaser_hip_icp_knn_search_batch", "teaser_hip_icp_hybrid_search_batch",
                 "teaser_hip_icp_radius_search_batch"):
        assert name in tp.EXPORTED_SYMBOLS
    for name in ("knn_search", "knn_search_batch", "hybrid_search", "hybrid_search_batch", "radius_search",
                 "radius_search_batch", "NearestNeighborSearch", "KDTreeFlann", "compute_point_cloud_distance",
                 "compute_nearest_neighbor_distance"):
        assert name in tp.__all__ and hasattr(tp, name)


def test_python_calls_check_arguments_and_have_no_cpu_path():
    P = np.random.default_rng(2).random((20, 3))
    with pytest.raises(ValueError, match="k must lie"):
        tp.knn_search(P, P, 101)
    with pytest.raises(ValueError, match="max_nn must lie"):
        tp.hybrid_search(P, P, 0.1, 0)
    with pytest.raises(ValueError, match="radius"):
        tp.hybrid_search(P, P, 0.0, 5)
    with pytest.raises(ValueError, match="radius"):
        tp.radius_search(P, P, float("nan"))
    with pytest.raises(ValueError, match="max_total"):
        tp.radius_search(P, P, 0.1, max_total=-1)
    with pytest.raises(ValueError, match="as many query sets"):
        tp.knn_search_batch([P, P], [P], 3)
    with pytest.raises(ValueError, match="n x 3"):
        tp.knn_search(P, np.zeros((4, 2)), 3)
    assert tp.compute_nearest_neighbor_distance(P[:1]).tolist() == [0.0]  # fewer than two points: zeros, no call
    assert tp.compute_nearest_neighbor_distance(np.zeros((0, 3))).shape == (0,)
    if tp.device_count() == 0:
        with pytest.raises(tp.TeaserHipError):
            tp.knn_search(P, P, 3)


def test_cxx_search_example_builds_and_fails_loudly_without_device():
    import subprocess

    from search_cxx import build_search_example
    exe = build_search_example()
    if tp.device_count() == 0:
        assert subprocess.call([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 77
