"""CPU checks of the yardstick above 2^16 correspondences (no GPU): the oracle's bitmap at n = 65 537 against the
reference expression evaluated in numpy on the rows and columns around the 16-bit boundary, and the long-N fixtures
of tests/golden/config_golden.json against the permuted problems they were made from."""
import hashlib
import importlib

import numpy as np
import pytest

from oracle import oracle
from util import LONG_N_PINNED, config_golden, long_n_permutation, long_n_problem, numpy_rows_predicate

tp = importlib.import_module("teaser-plusplus_amd")
LONG = ("long_65536", "long_65537", "long_100k")


def _bits(bm, rows, n):
    return np.unpackbits(np.ascontiguousarray(bm[rows]).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def test_oracle_bitmap_above_2_16_vs_numpy():
    """oracle.inlier_bitmap at n = 65 537 (the long_65537 fixture's problem): rows 0, 65 535, 65 536 and a sample of
    others bit for bit against numpy_rows_predicate, the columns 0, 65 535 and 65 536 of every row against the same
    rows (the graph is undirected), the padding bits of the last word zero, and the whole bitmap's SHA-256 and
    degree sum against the committed fixture."""
    fx = config_golden()["long_65537"]
    n, nb = fx["n"], fx["noise_bound"]
    pr = long_n_problem(tp, fx["seed"], n, fx["outlier_ratio"], nb)
    _, bm = oracle.inlier_bitmap(pr["src"], pr["dst"], nb, 1.0, False)
    assert bm.shape == (n, (n + 63) // 64) == (65537, 1025)
    assert hashlib.sha256(np.ascontiguousarray(bm).tobytes()).hexdigest() == fx["bitmap_sha256"]
    deg = np.bitwise_count(bm).sum(axis=1).astype(np.int64)
    assert int(deg.sum()) == fx["degree_sum"] == 2 * fx["num_edges"] and int(deg.max()) == fx["degree_max"]
    rng = np.random.default_rng(65537)
    edge = [0, 1, 63, 64, 65472, 65534, 65535, 65536]
    rows = np.unique(np.concatenate([edge, rng.choice(n, size=24, replace=False)]))
    want = numpy_rows_predicate(pr["src"], pr["dst"], rows, 2 * nb)
    assert (_bits(bm, rows, n) == want).all()
    for i in (0, 65535, 65536):
        col = ((bm[:, i >> 6] >> np.uint64(i & 63)) & np.uint64(1)).astype(bool)
        assert (col == numpy_rows_predicate(pr["src"], pr["dst"], [i], 2 * nb)[0]).all(), i
    assert not (bm[:, -1] >> np.uint64(1)).any()  # bits 65 537 .. 65 599 of every row
    # the three boundary indices are planted inliers: adjacent to each other
    assert want[np.searchsorted(rows, [0, 65535, 65536])][:, [0, 65535, 65536]].sum() == 6


@pytest.mark.parametrize("name", LONG)
def test_long_n_fixture_is_self_consistent(name):
    """The permutation is a product of disjoint swaps that puts 0, n - 1 (and 65 535 / 65 536 below n) into the
    planted inlier set, and the fixture's maximum clique is that set (the oracle's unique maximum; at 65 537 and
    100 000 one outlier consistent with every inlier joins it)."""
    fx = config_golden()[name]
    n = fx["n"]
    raw = tp.synth_problem(fx["seed"], n, fx["outlier_ratio"], fx["noise_bound"])
    perm = long_n_permutation(raw["inliers"])
    assert (perm[perm] == np.arange(n)).all()  # an involution
    moved = np.flatnonzero(perm != np.arange(n))
    assert len(moved) <= 2 * 4
    pr = long_n_problem(tp, fx["seed"], n, fx["outlier_ratio"], fx["noise_bound"])
    assert (pr["src"] == raw["src"][:, perm]).all() and (pr["dst"] == raw["dst"][:, perm]).all()
    inl = np.flatnonzero(pr["inliers"]).tolist()
    assert len(inl) == int(np.asarray(raw["inliers"]).sum())
    pinned = [i for i in LONG_N_PINNED + (n - 1,) if i < n]
    assert set(pinned) <= set(inl)
    assert fx["valid"] and fx["clique_unique"] and fx["long_n_permuted"]
    clique = fx["max_clique"]
    assert clique == sorted(clique) and set(inl) <= set(clique)
    assert len(clique) <= len(inl) + 1
    assert fx["num_edges"] * 2 == fx["degree_sum"]
    assert set(fx["translation_inliers"]) <= set(range(len(clique)))
