"""tests/outlier_reference.py (what the GPU's self k-NN and outlier removal are compared with) against an independently
written check: one stable argsort over the full distance matrix and straight Python loops for every sum; the seeded
cloud with planted far points loses exactly the planted ones; and what holds without a GPU for the Python calls."""
import importlib
import math

import numpy as np
import pytest

import outlier_reference as R

tp = importlib.import_module("teaser-plusplus_amd")


def loops_knn(P, k):
    n = len(P)
    D = np.empty((n, n))
    for i in range(n):
        for j in range(n):
            dx, dy, dz = P[i, 0] - P[j, 0], P[i, 1] - P[j, 1], P[i, 2] - P[j, 2]
            D[i, j] = (dx * dx + dy * dy) + dz * dz
    order = np.argsort(D, axis=1, kind="stable")  # stable: equal d2 keep ascending j
    m = min(k, n)
    idx = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf)
    idx[:, :m] = order[:, :m]
    d2[:, :m] = np.take_along_axis(D, order[:, :m], axis=1)
    return idx, d2


def loops_sum(values):
    total, nb = 0.0, (len(values) + 255) // 256
    for b in range(nb):
        s = 0.0
        for i in range(256 * b, min(256 * b + 256, len(values))):
            if values[i] is not None:
                s += values[i]
        total += s
    return total


def loops_statistical(P, nb, ratio):
    n = len(P)
    _, d2 = loops_knn(P, nb)
    m = min(nb, n)
    avg = []
    for i in range(n):
        acc = 0.0
        for t in range(m):
            acc += math.sqrt(d2[i, t])
        avg.append(acc / m)
    mean = loops_sum([a if a > 0 else None for a in avg]) / n
    ss = loops_sum([(a - mean) * (a - mean) if a > 0 else None for a in avg])
    std = math.sqrt(ss / (n - 1)) if n > 1 else float("nan")
    thr = mean + ratio * std
    keep = np.array([1 if (a > 0 and a < thr) else 0 for a in avg], dtype=np.uint8)
    return dict(keep=keep, avg=np.array(avg), mean=mean, std=std, threshold=thr)


def clouds():
    rng = np.random.default_rng(11)
    g = 0.25 * np.arange(4)
    lattice = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], 1)  # 64 points, massive ties
    dup = rng.random((70, 3))
    dup[10:40] = dup[3]
    return dict(lattice=lattice, random=rng.random((300, 3)) * [1.0, 2.0, 0.5], duplicates=dup,
                one=np.array([[0.5, 0.25, 0.125]]), blocks=rng.random((513, 3)))


@pytest.mark.parametrize("name", ["lattice", "random", "duplicates", "one"])
@pytest.mark.parametrize("k", [1, 7, 100])
def test_self_knn_equals_the_stable_argsort(name, k):
    P = clouds()[name]
    idx, d2 = R.self_knn(P, k, chunk=37)
    ridx, rd2 = loops_knn(P, k)
    assert np.array_equal(idx, ridx) and R.bits_equal(d2, rd2)


@pytest.mark.parametrize("name,nb,ratio", [("lattice", 7, 1.0), ("random", 20, 2.0), ("duplicates", 20, 2.0),
                                           ("duplicates", 40, 0.5), ("one", 5, 1.0), ("blocks", 3, 1.5),
                                           ("random", 1, 1.0)])
def test_statistical_equals_the_straight_loops(name, nb, ratio):
    P = clouds()[name]
    got, ref = R.statistical(P, nb, ratio), loops_statistical(P, nb, ratio)
    assert np.array_equal(got["keep"], ref["keep"]) and R.bits_equal(got["avg"], ref["avg"])
    assert R.bits_equal([got["mean"], got["std"], got["threshold"]], [ref["mean"], ref["std"], ref["threshold"]])


def test_consequences_of_the_rule():
    c = clouds()
    assert R.statistical(c["one"], 5, 1.0)["keep"].tolist() == [0]           # n = 1 keeps nothing
    assert not R.statistical(c["random"], 1, 1.0)["keep"].any()              # nb_neighbors = 1 keeps nothing
    s = R.statistical(c["duplicates"], 20, 2.0)                              # 31 copies of one point, 20 neighbours
    copies = [3] + list(range(10, 40))
    assert (s["avg"][copies] == 0).all() and not s["keep"][copies].any() and s["keep"].sum() > 0
    e = R.statistical(np.zeros((0, 3)), 5, 1.0)
    assert len(e["keep"]) == 0 and np.isnan(e["threshold"])


def test_radius_counts_are_strict_and_include_the_point():
    g = 0.25 * np.arange(4)
    lattice = np.stack([a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")], 1)
    r = R.radius(lattice, 1, 0.25)  # the six lattice neighbours sit at exactly the radius: excluded
    assert (r["count"] == 1).all() and not r["keep"].any()
    r = R.radius(lattice, 4, 0.25 * 1.0001)
    ref = np.array([sum(1 for q in lattice if ((p - q) ** 2).sum() < (0.25 * 1.0001) ** 2) for p in lattice])
    assert np.array_equal(r["count"], ref) and np.array_equal(r["keep"], (ref > 4).astype(np.uint8))
    assert r["count"].min() == 4 and r["count"].max() == 7


def test_planted_far_points_are_exactly_what_the_statistical_rule_drops():
    P, planted = R.planted_cloud()
    s = R.statistical(P, 20, 2.0)
    dropped = np.flatnonzero(s["keep"] == 0)
    assert dropped.tolist() == planted.tolist()
    # not a close call: the planted points' mean distances are far above the threshold, every other far below
    assert s["avg"][planted].min() > 2 * s["threshold"] and np.delete(s["avg"], planted).max() < 0.75 * s["threshold"]


def test_python_calls_check_arguments_and_have_no_cpu_path():
    for name in ("teaser_hip_icp_self_knn_batch", "teaser_hip_icp_remove_statistical_outliers_batch",
                 "teaser_hip_icp_remove_radius_outliers_batch", "teaser_hip_icp_set_option", "teaser_hip_icp_get_option"):
        assert name in tp.EXPORTED_SYMBOLS
    for name in ("remove_statistical_outlier", "remove_radius_outlier", "self_knn", "self_knn_batch",
                 "remove_statistical_outlier_batch", "remove_radius_outlier_batch"):
        assert name in tp.__all__
    P = clouds()["random"]
    with pytest.raises(ValueError, match="k must lie"):
        tp.self_knn(P, 101)
    with pytest.raises(ValueError, match="nb_neighbors"):
        tp.remove_statistical_outlier(P, 0, 2.0)
    with pytest.raises(ValueError, match="std_ratio"):
        tp.remove_statistical_outlier(P, 20, 0.0)
    with pytest.raises(ValueError, match="radius"):
        tp.remove_radius_outlier(P, 5, float("inf"))
    with pytest.raises(ValueError, match="nb_points"):
        tp.remove_radius_outlier(P, 0, 0.1)
    with pytest.raises(ValueError, match="one per cloud"):
        tp.self_knn_batch([P, P], [3, 4, 5])
    with pytest.raises(ValueError, match="n x 3"):
        tp.self_knn(np.zeros((4, 2)), 3)
    if tp.device_count() == 0:
        with pytest.raises(tp.TeaserHipError):
            tp.remove_statistical_outlier(P, 20, 2.0)


def test_cxx_outlier_example_builds_and_fails_loudly_without_device():
    import subprocess

    from outlier_cxx import build_outlier_example
    exe = build_outlier_example()
    if tp.device_count() == 0:
        assert subprocess.call([exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 77
