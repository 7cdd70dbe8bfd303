"""The Python forms of DBSCAN clustering (cluster_dbscan, cluster_dbscan_batch) on the contested-border scene of
tests/dbscan_reference.py against its hand-worked expectations: scalar and per-cloud arguments, the optional returns."""
import importlib

import numpy as np
import pytest

import dbscan_reference as RD

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def test_cluster_dbscan_single_cloud_and_optional_returns():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    for b_first in (False, True):
        P, eps, mp = RD.contested(b_first)
        labels, counts, roots, c = RD.contested_expected(b_first)
        got = tp.cluster_dbscan(P, eps, mp)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, labels)
        l2, c2 = tp.cluster_dbscan(P, eps, mp, return_counts=True)
        assert np.array_equal(l2, labels) and c2.dtype == np.int32 and np.array_equal(c2, counts)
        l3, r3 = tp.cluster_dbscan(P, eps, mp, return_roots=True)
        assert np.array_equal(l3, labels) and np.array_equal(r3, roots)
        l4, c4, r4 = tp.cluster_dbscan(P.astype(np.float32), eps, mp, return_counts=True, return_roots=True)
        assert np.array_equal(l4, labels) and np.array_equal(c4, counts) and np.array_equal(r4, roots)


def test_cluster_dbscan_batch_scalar_and_per_cloud_arguments():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")
    Pc, eps, mp = RD.contested(False)
    Pb = RD.contested(True)[0]
    ec, eb = RD.contested_expected(False), RD.contested_expected(True)
    labels, ncl = tp.cluster_dbscan_batch([Pc, np.zeros((0, 3)), Pb], eps, mp)
    assert ncl.dtype == np.int32 and ncl.tolist() == [2, 0, 2]
    assert np.array_equal(labels[0], ec[0]) and len(labels[1]) == 0 and np.array_equal(labels[2], eb[0])
    # per cloud: min_points 3 makes the contested point core (one cluster), eps 0 leaves no neighbours at all
    labels, ncl, counts, roots = tp.cluster_dbscan_batch([Pc, Pc, Pb], [eps, eps, 0.0], [mp, 3, mp],
                                                         return_counts=True, return_roots=True)
    assert ncl.tolist() == [2, 1, 0]
    assert np.array_equal(labels[0], ec[0]) and np.array_equal(counts[0], ec[1]) and np.array_equal(roots[0], ec[2])
    assert (labels[1] == 0).all() and (roots[1] == 0).all() and np.array_equal(counts[1], ec[1])
    assert (labels[2] == -1).all() and (counts[2] == 0).all() and (roots[2] == -1).all()
    labels, ncl, roots = tp.cluster_dbscan_batch([Pb], eps, [mp], return_roots=True)
    assert ncl.tolist() == [2] and np.array_equal(roots[0], eb[2])
    assert tp.cluster_dbscan_batch([], eps, mp)[0] == []
    with pytest.raises(ValueError):
        tp.cluster_dbscan_batch([Pc, Pb], [eps, eps, eps], mp)
    with pytest.raises(tp.TeaserHipError, match="min_points"):
        tp.cluster_dbscan(Pc, eps, 0)
