"""The restatement of DBSCAN clustering against itself (tests/dbscan_reference.py): the closed form equals a literal copy
of Open3D's loop whatever order its set is popped in, the hand-worked scenes give what was worked out by hand, and
sklearn's DBSCAN agrees wherever no pair lies at d2 == eps^2 (it tests <=, the contract <)."""
import numpy as np
import pytest

import dbscan_reference as RD


def test_closed_form_equals_the_literal_loop_on_random_lattices():
    rng = np.random.default_rng(2026)
    clusters = borders = 0
    for trial in range(60):
        n = int(rng.integers(1, 120))
        P = RD.random_lattice(rng, n, side=int(rng.integers(3, 8)))
        eps = [0.5, np.nextafter(0.5, np.inf), 0.75, 1.0, np.nextafter(1.0, np.inf)][trial % 5]
        mp = 1 + trial % 7
        A = RD.neighbours(P, eps)
        labels, counts, roots, c = RD.dbscan(P, eps, mp, A)
        assert np.array_equal(A, A.T) and A.diagonal().all()
        for _ in range(3):
            assert np.array_equal(RD.dbscan_literal(P, eps, mp, rng, A), labels)
        core = counts >= mp
        assert np.array_equal(roots >= 0, core) and c == len(np.unique(roots[core]))
        clusters += c
        borders += int(((labels >= 0) & ~core).sum())
    assert clusters > 60 and borders > 60


@pytest.mark.parametrize("name", sorted(RD.builders()))
def test_closed_form_equals_the_literal_loop_on_the_builders(name):
    P, eps, mp = RD.builders()[name]
    labels, counts, roots, c = RD.expected(name)
    rng = np.random.default_rng(len(name))
    assert np.array_equal(RD.dbscan_literal(P, eps, mp, rng, RD.adjacency(name)), labels)
    if len(P) < 1000:
        assert np.array_equal(RD.dbscan_literal(P, eps, mp, rng, RD.adjacency(name)), labels)
    assert c == (labels.max() + 1 if len(labels) else 0)


def test_hand_worked_scenes():
    for b_first in (False, True):
        P, eps, mp = RD.contested(b_first)
        got = RD.dbscan(P, eps, mp)
        want = RD.contested_expected(b_first)
        for g, w in zip(got[:3], want[:3]):
            assert np.array_equal(g, w)
        assert got[3] == want[3] == 2
    P, eps, mp = RD.touching(False)
    labels, counts, roots, c = RD.dbscan(P, eps, mp)
    assert c == 2 and labels.tolist() == [0] * 5 + [1] * 5 and roots.tolist() == [0] * 5 + [5] * 5
    assert counts.tolist() == [5] * 10  # the pairs at d2 == 1 are NOT neighbours
    P, eps, mp = RD.touching(True)
    labels, counts, roots, c = RD.dbscan(P, eps, mp)
    assert c == 1 and labels.tolist() == [0] * 10 and roots.tolist() == [0] * 10
    assert counts.tolist() == [5, 6, 5, 5, 6, 6, 5, 6, 5, 5]
    for order in ("ascending", "descending", "shuffled"):
        labels, counts, roots, c = RD.expected("chain_" + order)
        assert c == 1 and (labels == 0).all() and (roots == 0).all() and counts.min() == 2 and counts.max() == 3
    labels, _, roots, c = RD.expected("comb")
    assert c == 1 and (roots == 0).all()
    labels, counts, roots, c = RD.expected("identical")
    assert c == 1 and (counts == 513).all() and (roots == 0).all()
    # an eps whose square is not > 0: no neighbours at all
    labels, counts, roots, c = RD.dbscan(RD.lattice_slab(), 0.0, 1)
    assert c == 0 and (labels == -1).all() and (counts == 0).all() and (roots == -1).all()


def test_sklearn_agrees_where_no_pair_lies_on_the_radius():
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(7)
    compared = 0
    scenes = [(RD.random_lattice(rng, int(rng.integers(5, 120))), [0.6, 0.8, 1.1][t % 3], 1 + t % 6) for t in range(30)]
    scenes += [RD.builders()[k] for k in ("slab", "contested", "contested_b_first", "touching_joined", "flat", "shifted")]
    for P, eps, mp in scenes:
        e = P[:, None, :] - P[None, :, :]
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        if (d2 == eps * eps).any() or (np.sqrt(d2) == eps).any():
            continue
        sk = cluster.DBSCAN(eps=eps, min_samples=mp, algorithm="brute").fit(P)
        labels, counts, roots, c = RD.dbscan(P, eps, mp)
        core = np.zeros(len(P), dtype=bool)
        core[sk.core_sample_indices_] = True
        assert np.array_equal(core, counts >= mp)
        assert np.array_equal(sk.labels_, labels)  # also the contested border points: the first cluster wins there too
        compared += 1
    assert compared >= 20
