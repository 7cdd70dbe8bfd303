"""The three-launch degree closure (order, pairs, verdict) as a numpy model: the pair kernel's block rule -- row ballot,
lane accumulation, diagonal OR -- writes the FULL compact matrix, every word once, on every grid; and H from the full
rows by the rule of csrc/closure_h.h equals its definition.  No GPU."""
import numpy as np
import pytest

import closure_full_rows_model as M


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("m", M.SIZES)
def test_block_rule_reproduces_the_full_matrix_and_writes_every_word_once(m, kind):
    adj, _ = M.case(m, kind)
    ng = (m + 63) // 64
    expect = np.zeros((M.CORE_CAP, M.CORE_CAP // 64), np.int64)
    expect[:m, :ng] = 1
    pools = []
    for grid in M.GRIDS:
        pool, writes = M.pairs_launch(adj, grid)
        assert np.array_equal(writes, expect), (m, kind, grid)
        assert np.array_equal(M.unpack_rows(pool, m), adj), (m, kind, grid)
        # ranks >= m set no bit in any stored word
        tail = 64 * ng - m
        if tail:
            assert not (pool[:m, ng - 1] >> np.uint64(64 - tail)).any()
        pools.append(pool)
    assert all(np.array_equal(pools[0], p) for p in pools[1:])


@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("m", M.SIZES)
def test_h_from_full_rows_equals_the_definition(m, kind):
    adj, deg = M.case(m, kind)
    pool, _ = M.pairs_launch(adj, 16)
    assert np.array_equal(M.h_from_rows(pool, m, deg), M.h_definition(adj, deg))


def test_the_cases_reach_every_branch_of_the_rule():
    """below, above and the crossing block all occur, and the bench-like case has degrees that do not increase"""
    seen = set()
    for m in (129, 1000):
        for kind in M.KINDS:
            adj, deg = M.case(m, kind)
            pool, _ = M.pairs_launch(adj, 1)
            for v in range(0, m, 7):
                base = 0
                for B in range((m + 63) // 64):
                    w, cols = int(pool[v, B]), min(64, m - 64 * B)
                    if w:
                        cnt = bin(w).count("1")
                        seen.add("below" if base + cnt <= deg[64 * B + cols - 1] else
                                 "above" if base + 1 >= deg[64 * B] else "cross")
                        base += cnt
    assert seen == {"below", "above", "cross"}
    assert np.all(np.diff(M.case(1000, "bench")[1]) <= 0)
