"""A numpy model of tim_closure_pairs_kernel's output (csrc/kernels_graph.hip; CPU only): the partial compact rows of
the degree closure's candidate set R, evaluated from the points on the route whose K1 stores no row.

R = { deg >= t } comes from the oracle's degrees of a 600-point synthetic problem, ordered by (degree descending, vertex
ascending) as the order launch leaves it (keys = degree << 16 | vertex by rank).  The kernel writes word (a, b / 64), bit
b % 64, for the rank pairs its covering rule assigns to row a, evaluating the reference predicate on the two points; the
symmetrise launch computes full(a, b) = part(a, b) | part(b, a).  For both covering rules that were considered -- the
strict upper triangle by rank (the kernel's: a < b, blocks below the diagonal have no work) and the checkerboard (row a
takes {a, b} when (a < b) differs from the parity of a + b: equal work per row, but every block is evaluated) -- the
partial pool ORed with its transpose must equal the oracle's bitmap restricted to R x R, every unordered pair must be
covered exactly once, and the diagonal must be zero."""
import functools
import importlib

import numpy as np
import pytest

from oracle import oracle

tp = importlib.import_module("teaser-plusplus_amd")
N, NB, CORE_WORDS = 600, 0.01, 32
RULES = {
    "upper": lambda a, b: a < b,
    "checkerboard": lambda a, b: (a < b) != (((a + b) & 1) == 1),
}


@functools.lru_cache(maxsize=None)
def problem():
    pr = tp.synth_problem(20261200, N, 0.8, NB)
    src, dst = np.ascontiguousarray(pr["src"]), np.ascontiguousarray(pr["dst"])
    _, bm = oracle.inlier_bitmap(src, dst, NB, 1.0, False)
    dense = oracle.bitmap_to_dense(bm, N)
    deg = dense.sum(1)
    t = int(np.sort(deg)[::-1][199])  # R: the ~200 vertices of largest degree, ties included
    verts = [v for v in range(N) if deg[v] >= t]
    keys = sorted(((int(deg[v]) << 16) | v for v in verts), key=lambda k: (-(k >> 16), k & 0xffff))
    return src, dst, dense, keys


def edge(src, dst, u, v):
    """the reference predicate on two points: | |s_v - s_u| - |d_v - d_u| | <= beta, beta = 2 noise_bound"""
    a, b = src[:, v] - src[:, u], dst[:, v] - dst[:, u]
    A, B = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    return bool(abs(np.sqrt(A) - np.sqrt(B)) <= 2 * NB)


def partial_pool(rule):
    """[m, CORE_WORDS] uint64 as the kernel writes it, and how often each unordered pair was evaluated"""
    src, dst, _, keys = problem()
    m = len(keys)
    vert = [k & 0xffff for k in keys]
    part = np.zeros((m, CORE_WORDS), dtype=np.uint64)
    hits = np.zeros((m, m), dtype=int)
    for a in range(m):
        for b in range(m):
            if a == b or not rule(a, b):
                continue
            hits[min(a, b), max(a, b)] += 1
            if edge(src, dst, vert[a], vert[b]):
                part[a, b >> 6] |= np.uint64(1) << np.uint64(b & 63)
    return part, hits


def test_candidate_set_is_not_a_multiple_of_the_block():
    _, _, dense, keys = problem()
    m = len(keys)
    assert 200 <= m < 600 and m % 64 != 0 and m > 128  # several rank blocks, a ragged last one
    degs = [k >> 16 for k in keys]
    assert degs == sorted(degs, reverse=True)
    assert all(a < b for (da, a), (db, b) in zip([(k >> 16, k & 0xffff) for k in keys], [(k >> 16, k & 0xffff) for k in keys[1:]]) if da == db)


@pytest.mark.parametrize("rule", list(RULES))
def test_partial_pool_or_its_transpose_is_the_oracles_graph_on_r(rule):
    _, _, dense, keys = problem()
    m = len(keys)
    vert = np.array([k & 0xffff for k in keys])
    part, hits = partial_pool(RULES[rule])
    iu = np.triu_indices(m, 1)
    assert (hits[iu] == 1).all() and hits.sum() == m * (m - 1) // 2  # every unordered pair once
    bits = np.unpackbits(part.view(np.uint8), axis=1, bitorder="little")[:, :CORE_WORDS * 64].astype(bool)
    assert not bits[:, m:].any()                  # no column beyond |R|
    assert not bits[np.arange(m), np.arange(m)].any()  # the diagonal bit is zero
    full = bits[:, :m] | bits[:, :m].T
    assert (full == dense[np.ix_(vert, vert)]).all()
    if rule == "upper":  # the kernel's rule: a row's words in front of its diagonal block are zero, written as such
        for a in range(m):
            assert not part[a, :a >> 6].any() and not bits[a, :a + 1].any()
