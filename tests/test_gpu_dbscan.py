"""DBSCAN clustering on the MI355X (teaser_hip_icp_cluster_dbscan_batch through the Python form) against the numpy
restatement tests/dbscan_reference.py, whose neighbour sets are brute force (no grid): labels, neighbour counts, roots
and cluster counts, all integers, compared for EQUALITY.  Scenes: every builder of the restatement (the lattice slab,
the contested border in both index orders, the blob pair at exactly d2 == eps^2 and one ulp above, the 4 097-point chain
in three index orders and the comb -- union-find depth and the hook race --, 513 identical points -- every lane hooks at
one root --, the shifted and the flat cloud, a diagonal cluster that crosses cell boundaries on all three axes), each
with min_points 1 (every point core), its own middle value and n + 1 (all noise); the block edges 255 / 256 / 257; one
batch of sizes 0, 1, 257 and 4 097 with different records, reversed and each alone; the same call twice."""
import importlib

import numpy as np
import pytest

import dbscan_reference as RD

pytestmark = pytest.mark.gpu
tp = importlib.import_module("teaser-plusplus_amd")


def need_gpu():
    if tp.device_count() < 1:
        pytest.fail("the GPU suite needs an MI355X")


def run(clouds, eps, mp):
    labels, ncl, counts, roots = tp.cluster_dbscan_batch(clouds, eps, mp, return_counts=True, return_roots=True)
    return [(labels[b], counts[b], roots[b], int(ncl[b])) for b in range(len(clouds))]


def check(got, want, what):
    for g, w, part in zip(got, want, ("labels", "counts", "roots", "n_clusters")):
        assert np.array_equal(g, w), "%s: %s differ" % (what, part)


@pytest.mark.parametrize("name", sorted(RD.builders()))
def test_builders_equal_the_restatement(name):
    need_gpu()
    P, eps, mp = RD.builders()[name]
    mps = [1, mp, len(P) + 1]
    got = run([P] * 3, eps, mps)  # one call: the three records share the launches
    for g, m in zip(got, mps):
        want = RD.expected(name, m)
        check(g, want, "%s min_points %d" % (name, m))
    assert got[0][3] >= 1 and (got[0][0] >= 0).all()       # min_points 1: every point is core
    assert got[2][3] == 0 and (got[2][0] == -1).all()      # min_points n + 1: all noise
    assert (got[2][1] == got[0][1]).all()                   # the counts do not depend on min_points


@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_edges(n):
    need_gpu()
    P = RD.random_lattice(np.random.default_rng(n), n)
    want = RD.dbscan(P, 0.6, 4)
    assert want[3] >= 1 and (want[0] == -1).any()
    check(run([P], 0.6, 4)[0], want, "n %d" % n)


def test_batch_positions_and_repetition_give_identical_bits():
    need_gpu()
    rng = np.random.default_rng(99)
    clouds = [np.zeros((0, 3)), RD.random_lattice(rng, 1), RD.random_lattice(rng, 257), RD.chain("shuffled")[0]]
    eps = [0.5, 0.75, 0.6, 1.0]
    mp = [3, 1, 4, 3]
    want = [RD.dbscan(clouds[0], eps[0], mp[0]), RD.dbscan(clouds[1], eps[1], mp[1]),
            RD.dbscan(clouds[2], eps[2], mp[2]), RD.expected("chain_shuffled", 3)]
    assert want[3][3] == 1 and (want[3][2] == -1).sum() == 2  # min_points 3: the two chain ends are border points
    fwd = run(clouds, eps, mp)
    rev = run(clouds[::-1], eps[::-1], mp[::-1])[::-1]
    again = run(clouds, eps, mp)
    for b in range(4):
        check(fwd[b], want[b], "cloud %d in the batch" % b)
        alone = run([clouds[b]], eps[b], mp[b])[0]
        for other, what in ((rev[b], "reversed batch"), (again[b], "second call"), (alone, "alone")):
            for g, o in zip(fwd[b][:3], other[:3]):
                assert g.tobytes() == o.tobytes(), "cloud %d: %s" % (b, what)
            assert fwd[b][3] == other[3]


def test_refusals_name_the_argument():
    need_gpu()
    P, eps, mp = RD.contested()
    wide = RD.lattice_slab()  # an extent of 1e6 along x, of 2 and 0.5 along y and z: 41 + 25 + 23 key bits at eps 1e-7
    wide[0, 0] += 1e6
    for args, word in (((P, -1.0, mp), "eps"), ((P, float("nan"), mp), "eps"), ((P, 1e200, mp), "eps"),
                       ((P, eps, 0), "min_points"), ((wide, 1e-7, mp), "eps is too small")):
        with pytest.raises(tp.TeaserHipError, match=word):
            tp.cluster_dbscan(*args)
    check(run([P], eps, mp)[0], RD.contested_expected(), "after the refusals")
