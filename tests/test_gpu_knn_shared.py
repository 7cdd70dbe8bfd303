"""The self k-NN routes and the two-cloud k-NN search share one whole-cloud scan (csrc/icp_knn_device.h) and keep two
written-out ring kernels, the two-cloud one being the self one's general form; this test holds the two searches to the
same bits on a cloud searched in itself.  On one batch of clouds -- one and several blocks of 64 points, k below, at and above n, both
list capacities, and a cloud with two far outliers whose queries reach the worklist -- at "knn_ring_cap" 4 and 0:
self_knn_batch(P) and knn_search_batch(P, P) give the same bytes and the same "knn_fallbacks"; statistical removal and
k-NN normal estimation (with covariances and eigenvalues) give the same bytes at both ring caps; and all of them equal
the numpy restatements (tests/outlier_reference.py, tests/normals_reference.py) at the bars of tests/test_gpu_outlier.py
and tests/test_gpu_normals.py.  Normal estimation takes max_nn >= 3, so its k = 1 case runs with max_nn = 3."""
import importlib

import numpy as np
import pytest

import normals_reference as RN
import outlier_reference as RO
from test_gpu_normals import check as check_normals
from test_gpu_outlier import check_knn, check_statistical

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")
KS = [1, 32, 33, 100]
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def batch():
    rng = np.random.default_rng(77)
    clouds = [rng.random((n, 3)) for n in (1, 2, 63, 64, 65, 129)]
    far = rng.random((300, 3))
    far[17, 0], far[211, 1] = 1e3, 1e6
    return clouds + [far]


def at_both_caps(call):
    """(result, knn_fallbacks) of call() at ring cap 4 and at ring cap 0."""
    out = []
    try:
        for cap in (4, 0):
            tp.set_icp_option("knn_ring_cap", cap)
            got = call()
            out.append((got, tp.get_icp_option("knn_fallbacks")))
    finally:
        tp.set_icp_option("knn_ring_cap", 4)
    return out


def same_bytes(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("k", KS)
def test_self_knn_is_the_two_cloud_search_of_a_cloud_in_itself(k):
    clouds = batch()
    total = sum(len(c) for c in clouds)
    self_runs = at_both_caps(lambda: tp.self_knn_batch(clouds, k, return_distance=True))
    pair_runs = at_both_caps(lambda: tp.knn_search_batch(clouds, clouds, k))
    for cap, (s, s_fell), (p, p_fell) in zip((4, 0), self_runs, pair_runs):
        assert s_fell == p_fell and (s_fell == total if cap == 0 else s_fell < total)
        for P, a, b in zip(clouds, s, p):
            assert a[0].shape == (len(P), k) and same_bytes(a, b), "ring cap %d, n %d" % (cap, len(P))
    for P, a in zip(clouds, self_runs[0][0]):
        check_knn(P, k, got=a)
    for a, b in zip(self_runs[0][0], self_runs[1][0]):
        assert same_bytes(a, b)


@pytest.mark.parametrize("k", KS)
def test_statistical_removal_and_knn_normals_at_both_ring_caps(k):
    clouds = batch()
    stat = at_both_caps(lambda: tp.remove_statistical_outlier_batch(clouds, k, 1.5, return_stats=True))
    for (pts4, ind4, st4), (pts0, ind0, st0) in zip(stat[0][0], stat[1][0]):
        assert same_bytes((pts4, ind4, st4["avg"]), (pts0, ind0, st0["avg"]))
        assert RO.bits_equal([st4[s] for s in ("mean", "std", "threshold")], [st0[s] for s in ("mean", "std", "threshold")])
    for P, got in zip(clouds, stat[0][0]):
        check_statistical(P, k, 1.5, got=got)
    sp = tp.KDTreeSearchParamKNN(max(k, 3))
    nrm = at_both_caps(lambda: tp.estimate_normals_batch(clouds, sp, covariances=True, eigenvalues=True))
    assert nrm[1][1] == sum(len(c) for c in clouds)
    for P, a, b in zip(clouds, nrm[0][0], nrm[1][0]):
        assert same_bytes(a, b), "n %d" % len(P)
        key = (len(P), sp.max_nn)
        if key not in _refs:
            _refs[key] = RN.estimate_normals(P, sp.search, sp.radius, sp.max_nn, sp.orient, sp.ref)
        # (no bound on the share of points the 1e-6 rule excludes: one such point is over 1 % of a 63-point cloud)
        check_normals(a, _refs[key], "n %d max_nn %d" % key, ties=True)
